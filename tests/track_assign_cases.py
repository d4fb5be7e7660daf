"""Detection sequences for the tests of the optimal association: the crossing case that greedy loses, and a crowd of
heavily overlapping objects in which the greedy and the optimal tracker part ways.  Generated in float64 from fixed
seeds; a test rounds to its dtype once and gives the same values to the kernel and to the restatements."""
import functools

import numpy as np

from track_ref import F, iou

# x of the left edge of: detection c1, track A, detection c0, track B -- all 100 x 100 boxes on one line
_X = dict(c1=0.0, A=32.0, c0=57.0, B=84.0)
_SCORE = 0.9


def _box(x):
    return (x, 100.0, x + 100.0, 200.0)


def crossing_case():
    """frame 0 shows A and B (tracks 1 and 2, confirmed); frames 1 and 2 show c0 and c1 -> boxes [3, 2, 4] float32,
    scores [3, 2] float32, labels [3, 2] int64, count [3] int32"""
    boxes = np.array([[_box(_X["A"]), _box(_X["B"])], [_box(_X["c0"]), _box(_X["c1"])], [_box(_X["c0"]), _box(_X["c1"])]],
                     np.float32)
    return boxes, np.full((3, 2), _SCORE, np.float32), np.zeros((3, 2), np.int64), np.full(3, 2, np.int32)


def crossing_values():
    """the pair values of frame 1, [track A, track B] x [c0, c1]: iou * score in float32"""
    out = np.zeros((2, 2), np.float32)
    for i, t in enumerate("AB"):
        for j, c in enumerate(("c0", "c1")):
            out[i, j] = iou(tuple(F(v) for v in _box(_X[t])), tuple(F(v) for v in _box(_X[c]))) * F(_SCORE)
    return out


def crowded_sequence(frames=8, Q=40, objects=32, seed=3, side=220.0):
    """`objects` boxes of about 60 x 90 of one label that wander inside a side x side square, so that every box overlaps
    several others; now and then one is faint or hidden, and a few rows of clutter follow.  Rows are shuffled per frame.
    -> boxes [frames, Q, 4] float64, scores [frames, Q], labels [frames, Q] int64, count [frames] int32"""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((frames, Q, 4))
    scores = np.zeros((frames, Q))
    labels = np.zeros((frames, Q), np.int64)
    count = np.zeros(frames, np.int32)
    x, y = rng.uniform(0, side, objects), rng.uniform(0, side, objects)
    w, h = rng.uniform(50, 70, objects), rng.uniform(80, 100, objects)
    vx, vy = rng.uniform(-9, 9, objects), rng.uniform(-9, 9, objects)
    for f in range(frames):
        rows = []
        for k in range(objects):
            cx, cy = x[k] + vx[k] * f + rng.uniform(-4, 4), y[k] + vy[k] * f + rng.uniform(-4, 4)
            u = rng.random()
            if u < 0.06 and f:
                continue                                    # hidden
            sc = rng.uniform(0.3, 0.5) if u < 0.16 and f else rng.uniform(0.75, 0.98)
            rows.append(((cx - w[k] / 2, cy - h[k] / 2, cx + w[k] / 2, cy + h[k] / 2), sc, 0))
        for _ in range(3):
            cx, cy = rng.uniform(0, side, 2)
            rows.append(((cx - 30, cy - 45, cx + 30, cy + 45), rng.choice([0.9, 0.4]), int(rng.integers(0, 2))))
        rows = [rows[i] for i in rng.permutation(len(rows))][:Q]
        count[f] = len(rows)
        for j, (b, sc, lab) in enumerate(rows):
            boxes[f, j], scores[f, j], labels[f, j] = b, sc, lab
    return boxes, scores, labels, count


def run(cls, boxes, scores, labels, count, settings):
    """the sequence through a fresh restatement of class `cls` -> (ids [frames, Q] int32, the final State, the counters)"""
    ref = cls(settings)
    ids = np.stack([ref.update(boxes[f], scores[f], labels[f], count[f]) for f in range(len(count))])
    return ids, ref.state(), ref.log


@functools.lru_cache(maxsize=None)
def cached_crowd():
    return crowded_sequence()
