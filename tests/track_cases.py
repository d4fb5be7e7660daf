"""The scripted detection sequences of the tracking tests: objects on straight
paths with per-frame jitter that appear, hide and leave, clutter, duplicates, scores on the thresholds and rows a tracker
must ignore.  Everything is generated in float64 from a fixed seed; a test rounds it to its dtype once and gives the same
rounded values to the kernel and to `track_ref`."""
import functools

import numpy as np

from track_ref import TrackRef

# thresholds that fp16 and bf16 hold exactly, so that a score can sit exactly on each of them in every dtype
SETTINGS = dict(obj_score_thrs=dict(high=0.625, low=0.125), init_track_thr=0.75, num_frames_retain=3, num_tentatives=3,
                max_tracks=20)
NAN = float("nan")


def reference_sequence(frames=12, Q=48, objects=20, seed=7, s=SETTINGS):
    """-> boxes [frames, Q, 4] float64, scores [frames, Q] float64, labels [frames, Q] int64, count [frames] int32"""
    rng = np.random.default_rng(seed)
    high, low, init = s["obj_score_thrs"]["high"], s["obj_score_thrs"]["low"], s["init_track_thr"]
    boxes = np.zeros((frames, Q, 4))
    scores = np.zeros((frames, Q))
    labels = np.zeros((frames, Q), np.int64)
    count = np.zeros(frames, np.int32)
    cols, pitch = 5, 96.0
    obj = []
    for k in range(objects):
        w, h = rng.uniform(40, 72, 2)
        x, y = 24 + pitch * (k % cols), 24 + pitch * (k // cols)
        born = 0 if k < objects - 6 else int(rng.integers(1, 5))       # the last six appear later: tentative at first
        obj.append(dict(x=x, y=y, w=w, h=h, vx=rng.uniform(-3, 3), vy=rng.uniform(-3, 3), label=k % 3, born=born,
                        hidden=set(), faint=set(), gone=frames))
    obj[1]["hidden"] = {3}                 # one frame out of sight: found again by match A as a lost track
    obj[2]["hidden"] = {4, 5}
    obj[3]["gone"] = 4                     # leaves for good: retired after num_frames_retain frames
    obj[4]["hidden"] = {2, 3, 4, 5}        # away for longer than the tracker remembers: a new id on return
    obj[5]["faint"] = {2, 3, 6}            # a low score keeps it alive through match C
    obj[6]["faint"] = {5}
    obj[7]["hidden"], obj[7]["faint"] = {4}, {5}    # missed, then faint: match C takes no track that missed a frame
    for f in range(frames):
        rows = []
        for k, o in enumerate(obj):
            if f < o["born"] or f >= o["gone"] or f in o["hidden"]:
                continue
            cx, cy = o["x"] + o["vx"] * f + rng.uniform(-1, 1), o["y"] + o["vy"] * f + rng.uniform(-1, 1)
            w, h = o["w"] + rng.uniform(-1, 1), o["h"] + rng.uniform(-1, 1)
            sc = rng.uniform(0.3, 0.5) if f in o["faint"] else rng.uniform(0.8, 0.97)
            rows.append(((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), sc, o["label"]))
        if f in (1, 6):                    # exact duplicates of two rows: the match value of the pair ties
            rows += [rows[0], rows[5]]
        if f in (2, 7):                    # an overlapping box of another label on top of an object
            (x1, y1, x2, y2), sc, lab = rows[8]
            rows.append(((x1 + 2, y1 + 2, x2 + 2, y2 + 2), 0.9, (lab + 1) % 3))
        for _ in range(3):                 # clutter: one-frame boxes of high and of low score
            x, y = rng.uniform(0, 420, 2)
            w, h = rng.uniform(20, 60, 2)
            rows.append(((x, y, x + w, y + h), rng.choice([0.95, 0.85, 0.4, 0.2, 0.05]), int(rng.integers(0, 3))))
        # scores exactly on the thresholds, and what never takes part
        rows.append(((400.0, 400.0, 440.0, 450.0), high, 0))     # not above `high`: a low candidate
        rows.append(((300.0, 420.0, 330.0, 470.0), low, 1))      # not above `low`: nothing
        rows.append(((200.0, 430.0, 240.0, 480.0), init, 2))     # high, but not above `init_track_thr`: starts nothing
        rows.append(((10.0, 10.0, 10.0, 50.0), 0.9, 0))          # zero width
        rows.append(((10.0, 60.0, 50.0, 40.0), 0.9, 0))          # negative height
        rows.append(((NAN, 10.0, 50.0, 50.0), 0.9, 1))
        rows.append(((10.0, 10.0, 50.0, 50.0), NAN, 1))
        rows.append(((10.0, 10.0, float("inf"), 50.0), 0.9, 2))
        order = rng.permutation(len(rows))
        rows = [rows[i] for i in order][:Q]
        n = 0 if f == 9 else len(rows)     # one frame without a single detection
        count[f] = n
        for j, (b, sc, lab) in enumerate(rows):
            boxes[f, j], scores[f, j], labels[f, j] = b, sc, lab
        if f == 9:
            count[f] = 0
        # rows beyond the count hold what would start tracks if they were read
        for j in range(count[f], Q):
            boxes[f, j], scores[f, j], labels[f, j] = (50.0 + j, 50.0, 90.0 + j, 120.0), 0.99, 1
    return boxes, scores, labels, count


def dense_sequence(frames=3, Q=1024, seed=11):
    """the limits case: more than 512 track starts on frame 0 (a grid of small boxes that drift), then matches for all"""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((frames, Q, 4))
    scores = np.zeros((frames, Q))
    labels = np.zeros((frames, Q), np.int64)
    j = np.arange(Q)
    x, y = 4.0 + 14.0 * (j % 32), 4.0 + 14.0 * (j // 32)
    for f in range(frames):
        order = rng.permutation(Q) if f else j
        dx, dy = rng.uniform(-0.5, 0.5, Q), rng.uniform(-0.5, 0.5, Q)
        boxes[f, :, 0], boxes[f, :, 1] = (x + f + dx)[order], (y + dy)[order]
        boxes[f, :, 2], boxes[f, :, 3] = boxes[f, :, 0] + 10.0, boxes[f, :, 1] + 12.0
        scores[f] = rng.uniform(0.55, 0.99, Q) if f == 0 else rng.uniform(0.3, 0.99, Q)
        labels[f] = (j % 2)[order]
    return boxes, scores, labels, np.full(frames, Q, np.int32)


def run_reference(boxes, scores, labels, count, settings):
    """the sequence through a fresh TrackRef -> (ids [frames, Q] int32, the final State, the branch counters)"""
    ref = TrackRef(settings)
    ids = np.stack([ref.update(boxes[f], scores[f], labels[f], count[f]) for f in range(len(count))])
    return ids, ref.state(), ref.log


def assert_exercises_every_branch(log):
    """the reference sequence must take every branch of the rule, or a green test says little"""
    for key in ("A", "B", "C", "promoted", "tentative_removed", "retired", "refused", "tie", "started"):
        assert log[key] >= 1, f"the sequence never takes the branch {key!r}: {dict(log)}"


@functools.lru_cache(maxsize=None)
def cached_sequence(name):
    return {"reference": reference_sequence, "dense": dense_sequence,
            "second": functools.partial(reference_sequence, seed=23)}[name]()
