"""CPU: the numpy restatement of the appearance cue (tests/appearance_ref.py, include/codetr_appearance.h) on its own -- the
two sequences of tests/appearance_cases.py lose an id under the plain rule and keep it with the cue, for both
associations -- and what of the host side runs without a GPU: the settings, the Inferencer's argument checks, the binding's
table against the header."""
import ctypes
import functools
import os

import numpy as np
import pytest

import appearance_cases as cases
import appearance_ref
from appearance_ref import TrackAppRef, TrackAssignAppRef, describe
from track_motion_sim_ref import TrackAssignMotionSimRef, TrackMotionSimRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = dict(greedy=TrackAppRef, optimal=TrackAssignAppRef)


@functools.lru_cache(maxsize=None)
def _sequence(name):
    frames, dets, names = cases.sequence(name)
    descs = [describe(img, np.array(b, np.float32).reshape(-1, 4)) for img, b in zip(frames, dets)]
    for d in descs:
        d.setflags(write=False)
    return frames, dets, names, descs


def _run(ref, name, appearance):
    _, dets, _, descs = _sequence(name)
    rows = []
    for b, d in zip(dets, descs):
        b = np.array(b, np.float32).reshape(-1, 4)
        rows.append(ref.update(b, np.full(len(b), 0.9, np.float32), np.zeros(len(b), np.int64),
                               desc=d if appearance else None).tolist())
    return rows


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_reentry(association):
    names = _sequence("reentry")[2]
    plain = REFS[association]()
    rows = _run(plain, "reentry", False)
    assert plain.issued == 3 and rows[14] == [1, -3] and rows[-1] == [1, 3]     # the red object returns as a new, tentative id
    ref = REFS[association]()
    rows = _run(ref, "reentry", True)
    assert ref.issued == 2 and ref.log["gated"] == 1
    assert all(r == ([1, 2] if len(n) == 2 else [1]) for r, n in zip(rows, names))
    assert sum(len(n) == 2 for n in names) == 16


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_lanes(association):
    names = _sequence("lanes")[2]
    plain = REFS[association]()
    rows = _run(plain, "lanes", False)
    assert all(r == [1, 3, 2] for r in rows[16:]) and all(r == [1, 2, 3] for r in rows[:8])   # the ids have swapped
    ref = REFS[association]()
    rows = _run(ref, "lanes", True)
    assert ref.issued == 3 and ref.log["gated"] == 2
    assert all(r == ([1, 2, 3] if len(n) == 3 else [1]) for r, n in zip(rows, names))


def test_stripes_sum_to_256_and_other_rows_are_zero():
    for Hh, Ww, seed in ((48, 64, 1), (37, 53, 2)):
        img = cases.edge_image(Hh, Ww, seed)
        boxes = np.array(cases.geometry_boxes(Hh, Ww) + [(1e30, 2.0, 3e38, 9.0), (-3e38, -3e38, 3e38, 3e38)], np.float32)
        d = describe(img, boxes, len(boxes) - 1)
        part = [appearance_ref.participates(b) for b in boxes]
        assert sum(part) == 14 and not part[11] and not part[14]
        for q, p in enumerate(part):
            sums = d[q].reshape(2, 64).sum(axis=1).tolist()
            assert sums == ([256, 256] if p and q < len(boxes) - 1 else [0, 0]), (q, sums)
    # a solid colour falls into one bin of each stripe; the bin edges are at 64, 128, 192
    img = np.zeros((40, 40, 3), np.uint8)
    img[:20] = (63, 64, 255)
    img[20:] = (192, 127, 128)
    d = describe(img, np.array([(0, 0, 40, 40)], np.float32))[0]
    assert d[0 * 16 + 1 * 4 + 3] == 256 and d[64 + 3 * 16 + 1 * 4 + 2] == 256 and d.sum() == 512
    assert not describe(img, np.array([(0, 0, 40, 40)], np.float32), 0).any()


def test_without_descriptors_it_is_the_tracker_as_it_is():
    """desc=None restates track_motion_sim_ref exactly, motion rows included"""
    _, dets, _, _ = _sequence("lanes")
    motions = [None, (1.5, -2.0, 1, 1, 1, 0, 0, 0), (2.0, 1.0, 1, 2, 1.01, 0.004, 80, 60), (0, 0, 0, 0, 0, 0, 0, 0)]
    for new, old in ((TrackAppRef, TrackMotionSimRef), (TrackAssignAppRef, TrackAssignMotionSimRef)):
        a, b = new(), old()
        for f, boxes in enumerate(dets):
            boxes = np.array(boxes, np.float32).reshape(-1, 4)
            args = (boxes, np.full(len(boxes), 0.9, np.float32), np.zeros(len(boxes), np.int64))
            assert a.update(*args, motion=motions[f % 4]).tolist() == b.update(*args, motion=motions[f % 4]).tolist()
        sa, sb = a.state(), b.state()
        assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(sa[3:], sb[3:]))
        assert sa[:3] == sb[:3] and not a.g.any()


def test_blend_adopt_and_the_similarity():
    g = np.zeros(128, np.uint16)
    d = np.zeros(128, np.uint16)
    d[5], d[70] = 256, 256
    assert appearance_ref.similarity(g, d) == 0
    g = (16 * d.astype(np.int64)).astype(np.uint16)
    assert appearance_ref.similarity(g, d) == 1 and g.max() == 4096
    e = np.zeros(128, np.uint16)
    e[5], e[6], e[70] = 128, 128, 256
    assert appearance_ref.similarity(g, e) == np.float32(0.75)
    blended = (7 * g.astype(np.int64) + 16 * e.astype(np.int64) + 4) >> 3
    assert blended[5] == (7 * 4096 + 2048 + 4) >> 3 and blended[6] == (2048 + 4) >> 3 and blended[70] == 4096


def test_settings():
    from codetr import hip_ops

    assert hip_ops.APPEARANCE == dict(appearance_thr=0.75, proximity_thr=0.5, reid_gate=1.5) == appearance_ref.DEFAULTS
    assert hip_ops.appearance_settings() == hip_ops.APPEARANCE and hip_ops.appearance_settings() is not hip_ops.APPEARANCE
    assert hip_ops.appearance_settings(dict(reid_gate=0, appearance_thr=1)) == dict(appearance_thr=1.0, proximity_thr=0.5,
                                                                                  reid_gate=0.0)
    for bad in (dict(gate=1), dict(appearance_thr=1.01), dict(appearance_thr=-0.1), dict(proximity_thr=2), dict(reid_gate=-1),
                dict(proximity_thr=float("nan")), dict(reid_gate=float("inf")), dict(appearance_thr="0.5"),
                dict(proximity_thr=True)):
        with pytest.raises(ValueError):
            hip_ops.appearance_settings(bad)


def test_inferencer_arguments():
    from codetr.inferencer import track_appearance_settings

    tracker = dict(max_tracks=8)
    assert track_appearance_settings(None, None) is None and track_appearance_settings(None, tracker) is None
    assert track_appearance_settings("color", tracker) == dict(appearance_thr=0.75, proximity_thr=0.5, reid_gate=1.5)
    assert track_appearance_settings(dict(type="color", reid_gate=2), tracker)["reid_gate"] == 2.0
    with pytest.raises(ValueError):
        track_appearance_settings("color", None)                       # no tracker
    for bad in ("colour", "reid", dict(appearance_thr=0.5), dict(type="color", thr=1), dict(type="color", reid_gate=-1), 1):
        with pytest.raises(ValueError):
            track_appearance_settings(bad, tracker)


def test_header_and_binding():
    from codetr import _appearance, _cabi, _cheader, _motion

    text = open(os.path.join(ROOT, "include", "codetr_appearance.h")).read()
    functions, defines = _cheader.parse(text)
    assert list(functions) == ["codetr_appearance_abi_version", "codetr_appearance_state_bytes", "codetr_appearance_work_bytes",
                               "codetr_appearance_describe_f16", "codetr_appearance_describe_bf16",
                               "codetr_appearance_describe_f32", "codetr_track_update5_f16", "codetr_track_update5_bf16",
                               "codetr_track_update5_f32"]
    assert defines == dict(CODETR_APPEARANCE_ABI_VERSION=1, CODETR_APPEARANCE_BINS=128, CODETR_APPEARANCE_COLS=16,
                           CODETR_APPEARANCE_ROWS=32)
    assert set(_appearance.SIGNATURES) == set(functions) and _appearance.ABI_VERSION == 1 and _appearance.BINS == 128
    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _appearance.SIGNATURES["codetr_appearance_abi_version"] == (i, [])
    assert _appearance.SIGNATURES["codetr_appearance_state_bytes"] == (l, [l])
    assert _appearance.SIGNATURES["codetr_appearance_work_bytes"] == (l, [l, l, l])
    for suffix in ("f16", "bf16", "f32"):
        assert _appearance.SIGNATURES["codetr_appearance_describe_" + suffix] == (i, [p, p, l, l, p, p, p, l, p])
        old = _motion.SIGNATURES["codetr_track_update4_" + suffix]     # update4's arguments, then the five of the cue
        assert _appearance.SIGNATURES["codetr_track_update5_" + suffix] == (old[0], old[1] + [p, p, p, p, l])
        params = functions["codetr_track_update5_" + suffix][1]
        assert [n for _, n in params[:-5]] == [n for _, n in _motion.functions["codetr_track_update4_" + suffix][1]]
        assert [n for _, n in params[-5:]] == ["desc_dev", "app_state_dev", "app_settings_host", "work_dev", "work_bytes"]
    assert not set(functions) & (set(_cabi.SIGNATURES) | set(_motion.SIGNATURES))   # a companion: the others are untouched
    assert _motion.ABI_VERSION == 2
    for phrase in ("HARD 2-bit colour", "no spatial layout beyond two stripes", "NOTHING is learned",
                   "has the other's colours", "parity with BoT-SORT / FastReID is unpinned", "(7 g[k] + 16 d[k] + 4) >> 3",
                   "u_i = (float)(6 i + 19) / 128.0f", "value = v + s when near && s >= appearance_thr"):
        assert phrase in text, phrase
