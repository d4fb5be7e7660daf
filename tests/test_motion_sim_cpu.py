"""CPU: the numpy restatement of the similarity camera-motion rule (tests/motion_sim_ref.py; include/codetr_motion.h,
version 2) on its own -- it recovers known zooms and rolls, it falls back to the translation rule's very floats where the
rule says so, and with it the tracker reference keeps the ids of eight small boxes over a zooming, rolling camera that costs
the uncompensated and the translation-compensated tracker all of them."""
import numpy as np
import pytest

import motion_cases
import motion_ref
import motion_sim_cases as cases
import motion_sim_ref
from track_motion_ref import TrackMotionRef
from track_motion_sim_ref import TrackMotionSimRef
from track_ref import TrackRef

# max(|a - truth|, |b - truth|) over the nine steps of motion_sim_cases.STEPS: twice the restatement's own worst error on
# these committed frames (measured: k2 0.00108 / 0.00550 with the foreground, sq 0.00075 / 0.00198, k1 0.00197 / 0.00384)
BOUNDS = {("k2", False): 0.0022, ("k2", True): 0.0110, ("sq", False): 0.0015, ("sq", True): 0.0040,
          ("k1", False): 0.0040, ("k1", True): 0.0077}


def _bits(values):
    return np.array([float(v) for v in values], np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("name,foreground", sorted(BOUNDS))
def test_recovers_zoom_and_roll(name, foreground):
    ref = motion_sim_ref.MotionSimRef()
    worst = 0.0
    for f, (img, step) in enumerate(zip(cases.frames(name, cases.STEPS, foreground), cases.STEPS)):
        motion, diag = ref.estimate(img)
        if f == 0:
            assert motion == motion_sim_ref.ZERO8 and diag[2:] == (0, 0, 0, 0, -1, -1)
            continue
        a, b = cases.truth(step)
        err = max(abs(float(motion[4]) - a), abs(float(motion[5]) - b))
        print(name, foreground, f, [float(v) for v in motion], diag, f"{err:.5f}")
        assert motion[2] == 1 and motion[3] == 2 and all(v.dtype == np.float32 for v in motion)
        assert diag[5] >= 4 and 2 * diag[5] >= diag[2] and 0 <= diag[6] < diag[7] < diag[2]
        worst = max(worst, err)
    print(name, foreground, "worst", worst)
    assert worst <= BOUNDS[name, foreground]
    assert (ref.k, diag[1]) == {"k1": (1, 35), "k2": (2, 35), "sq": (2, 81)}[name]


def test_a_pure_pan_gives_the_translation():
    """within a hundredth of a pixel of the translation rule's dx, dy; a = 1, b = 0 within the k2 bound"""
    sim, tra = motion_sim_ref.MotionSimRef(), motion_ref.MotionRef()
    for f, (img, step) in enumerate(zip(cases.frames("k2", cases.PURE_PANS), cases.PURE_PANS)):
        m, d = sim.estimate(img)
        (dx, dy, valid), _ = tra.estimate(img)
        if f == 0:
            continue
        print(f, [float(v) for v in m], d, float(dx), float(dy))
        assert valid == 1 and m[3] == 2
        assert abs(float(m[0]) - float(dx)) <= 0.01 and abs(float(m[1]) - float(dy)) <= 0.01
        assert abs(float(m[0]) - step[2][0]) <= 1.0 and abs(float(m[1]) - step[2][1]) <= 1.0       # half a cell at k = 2
        assert abs(float(m[4]) - 1) <= BOUNDS["k2", False] and abs(float(m[5])) <= BOUNDS["k2", False]


def _fallback(frames, settings=None):
    """the rows of both restatements over the frames; a row of the similarity one that is no similarity must be the
    fallback of the other's"""
    sim, tra = motion_sim_ref.MotionSimRef(settings), motion_ref.MotionRef(settings)
    rows = []
    for img in frames:
        m, d = sim.estimate(img)
        (dx, dy, valid), dt = tra.estimate(img)
        assert d[:4] == dt
        if m[3] != 2:
            want = (dx, dy, 1, 1, 1, 0, 0, 0) if valid == 1 else (0,) * 8
            assert _bits(m) == _bits(want)
        rows.append((m, d))
    assert np.array_equal(sim.state_bytes(), tra.state_bytes())
    return rows


def test_fallback_rows_are_the_translation_rule_s():
    k2 = motion_cases.recover_frames("k2", ((0, 0), (2, 0), (-2, 2)))
    rows = _fallback(k2, dict(grid=32, search=1, min_blocks=1))            # one block: no pair
    assert rows[1][1] == (8, 1, 1, 1, 0, 0, -1, -1) and [m[3] for m, _ in rows] == [0, 1, 1]
    flat = np.full((192, 256, 3), 90, np.uint8)
    small = motion_cases.texture(3, 30, 30, 4)
    # a flat frame behind a textured one: every block votes (0, 0), the identity is a valid similarity; the frame behind
    # the flat one has no textured block; then size changes and a frame without blocks
    rows = _fallback([k2[0], flat, k2[0], small, small, k2[0]])
    assert [m[3] for m, _ in rows] == [0, 2, 0, 0, 0, 0] and rows[2][1] == (2, 35, 0, 0, 0, 0, -1, -1)
    assert _bits(rows[1][0]) == _bits((0, 0, 1, 2, 1, 0, 128, 96))
    far = motion_cases.recover_frames("k2", ((0, 0), (40, 0), (0, 0)))     # a pan of 40 px at a reach of 16
    sim, tra = motion_sim_ref.MotionSimRef(), motion_ref.MotionRef()
    for img in far[:2]:
        m, d = sim.estimate(img)
        t, _ = tra.estimate(img)
    print("beyond the reach", [float(v) for v in m], d, t)
    if m[3] != 2:                                                           # (whichever it is, it is the rule's)
        assert _bits(m[:3]) == _bits(t)


def test_one_row_of_collinear_blocks_is_a_valid_similarity():
    ref = motion_sim_ref.MotionSimRef()
    for f, (img, step) in enumerate(zip(cases.frames("row", cases.STEPS[:4]), cases.STEPS[:4])):
        m, d = ref.estimate(img)
        if f:
            a, b = cases.truth(step)
            print(f, [float(v) for v in m], d, a, b)
            assert d[:3] == (3, 5, 5) and m[3] == 2 and d[5] >= 4
            assert abs(float(m[4]) - a) <= 0.02 and abs(float(m[5]) - b) <= 0.02


def test_search_ties_and_eligibility():
    """blocks of one row with equal votes: every pair at least two blocks apart is eligible and has all blocks as inliers;
    the lowest (i, j) wins.  Neighbours alone: no eligible pair."""
    g = [(x, 0) for x in range(5)]
    V = [(16, -16)] * 5
    assert motion_sim_ref.search(g, V, 8)[:4] == (6, 5, 0, 2)
    assert motion_sim_ref.search(g[:2], V[:2], 8)[:4] == (0, 0, -1, -1)
    assert motion_sim_ref.search([(0, 0), (1, 1)], V[:2], 8)[:4] == (0, 0, -1, -1)     # |D|^2 = 2
    # a zoom of 1 + 32 / 512 about block 0: the block at (1, 1) should move by (16, 16); (16, 0) is one cell off and still
    # an inlier, (16, -1) is not
    assert motion_sim_ref.search([(0, 0), (2, 0), (1, 1)], [(0, 0), (32, 0), (16, 0)], 8)[:4] == (1, 3, 0, 1)
    assert motion_sim_ref.search([(0, 0), (2, 0), (1, 1)], [(0, 0), (32, 0), (16, -1)], 8)[:4] == (1, 2, 0, 1)


def test_the_eight_boxes_keep_their_ids_only_with_the_similarity():
    boxes, scores, labels, count = cases.scene_boxes()
    est, est_t = motion_sim_ref.MotionSimRef(), motion_ref.MotionRef()
    plain, shifted, comp = TrackRef(), TrackMotionRef(), TrackMotionSimRef()
    for f, img in enumerate(cases.box_frames()):
        motion, _ = est.estimate(img)
        ids = comp.update(boxes[f], scores[f], labels[f], count[f], motion=motion).tolist()
        assert ids == [1, 2, 3, 4, 5, 6, 7, 8], (f, ids)
        plain.update(boxes[f], scores[f], labels[f], count[f])
        shifted.update(boxes[f], scores[f], labels[f], count[f], motion=est_t.estimate(img)[0])
    print("ids issued: plain", plain.issued, "translation", shifted.issued, "similarity", comp.issued)
    assert plain.issued > 8 and shifted.issued > 8 and comp.issued == 8
