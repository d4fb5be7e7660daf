"""CPU: the numpy restatement of the camera-motion rule (tests/motion_ref.py, include/codetr_motion.h) on its own -- it
recovers known pans, it declares the frames invalid that the rule says are, and with it the tracker reference keeps its
ids over a jerky pan that costs the uncompensated one all of them."""
import numpy as np
import pytest

import motion_cases
import motion_ref
from track_motion_ref import TrackMotionRef
from track_ref import TrackRef


@pytest.mark.parametrize("name", sorted(motion_cases.RECOVER))
def test_recovers_integer_pans_under_noise_and_a_foreground(name):
    """bound: 0.5 cell per axis (the nearest-cell decision is what the tracker needs, the sub-cell step is a refinement).
    Measured maxima on these inputs: k1 0.06, k2 0.12, k3 0.33 cell (k3 has five blocks in all)."""
    pans = motion_cases.recover_pans(name)
    ref = motion_ref.MotionRef()
    worst = 0.0
    for f, (img, (px, py)) in enumerate(zip(motion_cases.recover_frames(name, pans), pans)):
        (dx, dy, valid), (k, blocks, n, c) = ref.estimate(img)
        if f == 0:
            assert valid == 0 and blocks >= 4
            continue
        assert valid == 1 and n >= 4 and 2 * c >= n
        assert dx.dtype == dy.dtype == np.float32
        err = max(abs(float(dx) - px), abs(float(dy) - py)) / k
        worst = max(worst, err)
        print(name, f, (px, py), float(dx), float(dy), (k, blocks, n, c), f"{err:.3f} cell")
        assert err <= 0.5
    print(name, "worst", worst)
    assert ref.k == {"k1": 1, "k2": 2, "k3": 3}[name]


def test_invalid_frames_and_the_state_after_them():
    textured = motion_cases.pan_frames()[0]
    ref = motion_ref.MotionRef()
    zero = (np.float32(0), np.float32(0), np.float32(0))

    def check_state(img):
        k, thumb = motion_ref.thumbnail(img, 160)
        raw = ref.state_bytes()
        assert raw[:16].view(np.int32).tolist() == [1, img.shape[0], img.shape[1], k]
        assert np.array_equal(raw[16:16 + thumb.size], thumb.reshape(-1)) and not raw[16 + thumb.size:].any()

    assert not ref.state_bytes().any()                                   # fresh: all zero
    motion, diag = ref.estimate(textured)                                # a first frame
    assert motion == zero and diag == (2, 35, 0, 0)
    check_state(textured)
    motion, diag = ref.estimate(textured)
    assert motion == (0, 0, 1) and diag == (2, 35, 35, 35)
    flat = np.full((192, 256, 3), 90, np.uint8)                          # nothing to match: the previous frame is flat
    ref.estimate(flat)
    check_state(flat)
    motion, diag = ref.estimate(textured)
    assert motion == zero and diag == (2, 35, 0, 0)
    check_state(textured)
    small = motion_cases.texture(3, 30, 30, 4)                           # a size change, and no blocks
    motion, diag = ref.estimate(small)
    assert motion == zero and diag == (1, 0, 0, 0)
    check_state(small)
    motion, diag = ref.estimate(small)                                   # the same size again: still no blocks
    assert motion == zero and diag == (1, 0, 0, 0)
    motion, diag = ref.estimate(textured)                                # back: a size change
    assert motion == zero and diag == (2, 35, 0, 0)
    check_state(textured)


def test_floor_division_of_the_step():
    assert motion_ref.step(10, 4, 12) == (16 * -2 + 14) // 28 == -1       # a negative numerator rounds down
    assert motion_ref.step(12, 4, 10) == 1 and motion_ref.step(5, 5, 5) == 0 and motion_ref.step(0, 0, 100) == -8


def test_ties_go_to_the_smallest_displacement():
    S = np.full((17, 17), 50)
    S[8 + 2, 8 - 3] = S[8 - 2, 8 + 3] = S[8 + 3, 8 + 2] = 7               # 13, 13, 13: the lowest dy
    S[8 - 4, 8] = 7                                                        # 16
    assert motion_ref.vote(S, 8) == (16 * 3, 16 * -2)                      # (equal neighbours: no sub-cell step)
    S[8 + 2, 8 + 3] = 7                                                    # 13 again, dy = 2: the lowest dx wins there
    S[8 - 2, 8 + 3] = 50
    assert motion_ref.vote(S, 8) == (16 * -3, 16 * 2)
    S[8, 8 + 1] = 7                                                        # 1
    assert motion_ref.vote(S, 8) == (16, 0)


def test_jerky_pan_keeps_ids_only_with_the_motion():
    boxes, scores, labels, count = motion_cases.pan_boxes()
    est, plain, comp = motion_ref.MotionRef(), TrackRef(), TrackMotionRef()
    worst = 0.0
    for f, (img, pan) in enumerate(zip(motion_cases.pan_frames(), motion_cases.PANS)):
        motion, _ = est.estimate(img)
        if f:
            assert motion[2] == 1
            worst = max(worst, abs(float(motion[0]) - pan[0]), abs(float(motion[1]) - pan[1]))
        got = comp.update(boxes[f], scores[f], labels[f], count[f], motion=motion).tolist()
        assert got == [1, 2, 3, 4, 5, 6], f
        ids = plain.update(boxes[f], scores[f], labels[f], count[f]).tolist()
        if f in (3, 5, 6, 8):
            assert all(i < -6 for i in ids), (f, ids)                     # only fresh, tentative ids
        else:
            assert ids == [1, 2, 3, 4, 5, 6], (f, ids)
    assert worst <= 0.1                                                   # measured 0.06 px on this sequence
    assert plain.issued == 24 and comp.issued == 6
