"""GPU: the camera-motion kernels (csrc/motion.hip), `codetr_track_update3_*` and the Inferencer's `track_motion` against
the numpy restatements (tests/motion_ref.py, tests/track_motion_ref.py), bit for bit -- the motion floats, the diag ints,
the state bytes, the ids of every row and the whole decoded track state.  The motion states sit between sentinel-filled
guard rows."""
import functools

import numpy as np
import pytest
import torch

import motion_cases
import motion_ref
import track_cases
from test_inferencer_batch_gpu import DEV, SWIN, _same
from test_track_gpu import _assert_state
from track_motion_ref import TrackAssignMotionRef, TrackMotionRef

pytestmark = pytest.mark.gpu
SENTINEL_BYTE = 0xA5
PANS8 = ((0, 0), (6, 0), (-5, 3), (2, -7), (0, 0), (-4, -4), (7, 5), (-3, 2))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _reference(frames, streams, settings, S):
    """-> (motion [N, 4] float32, diag [N, 4] int32, states [S, bytes] uint8) of the restatement"""
    refs = [motion_ref.MotionRef(settings) for _ in range(S)]
    motion, diag = np.zeros((len(frames), 4), np.float32), np.zeros((len(frames), 4), np.int32)
    for n, (img, s) in enumerate(zip(frames, streams)):
        m, d = refs[s].estimate(img)
        motion[n, :3], diag[n] = m, d
    return motion, diag, np.stack([r.state_bytes() for r in refs])


class Device:
    """S motion states between two guard rows; `run` feeds the frames in launches of `chunks` rows"""

    def __init__(self, S):
        from codetr import hip_ops

        self.all = hip_ops.new_motion_state(S + 2, DEV)
        self.all[0].fill_(SENTINEL_BYTE)
        self.all[-1].fill_(SENTINEL_BYTE)
        self.state = self.all[1:-1]

    def run(self, frames, streams, settings, chunks=None):
        from codetr import hip_ops

        motion, diag, at = [], [], 0
        for n in chunks or [len(frames)]:
            part = frames[at:at + n]
            sizes = [im.size for im in part]
            offsets = np.cumsum([0] + sizes).tolist()
            buf = torch.from_numpy(np.concatenate([im.reshape(-1) for im in part])).to(DEV)
            rows = [(o, im.shape[0], im.shape[1]) for o, im in zip(offsets, part)]
            m, d = hip_ops.estimate_motion(buf, rows, self.state, streams[at:at + n], settings)
            motion.append(m.cpu().numpy())
            diag.append(d.cpu().numpy())
            at += n
        assert at == len(frames)
        raw = self.all.cpu().numpy()
        assert (raw[0] == SENTINEL_BYTE).all() and (raw[-1] == SENTINEL_BYTE).all()   # the guard rows
        return np.concatenate(motion), np.concatenate(diag), raw[1:-1]


def _check(frames, streams=None, settings=None, S=1, chunks=None):
    streams = streams or [0] * len(frames)
    want = _reference(frames, streams, settings, S)
    got = Device(S).run(list(frames), streams, settings, chunks)
    print("motion", got[0].tolist(), "diag", got[1].tolist())
    assert np.array_equal(got[1], want[1]), "diag"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), "motion"
    assert np.array_equal(got[2], want[2]), "state"
    return got


# ---- 1. the estimate --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(motion_cases.RECOVER))
def test_three_sizes(name):
    """k = 1, 2 and 3 (with remainders on both axes), noise and a foreground that moves its own way"""
    frames = motion_cases.recover_frames(name, PANS8)
    motion, diag, _ = _check(frames)
    k = diag[0, 0]
    assert k == {"k1": 1, "k2": 2, "k3": 3}[name] and motion[0, 2] == 0 and (motion[1:, 2] == 1).all()
    assert np.abs(motion[1:, :2] - np.array(PANS8[1:], np.float32)).max() <= 0.5 * k   # the CPU test's bound


@functools.lru_cache(maxsize=None)
def _stripes():
    """vertical stripes of a 4-pixel period, moved by one pixel: sums that tie four cells apart and along the stripes"""
    x = np.arange(131 + 8)
    row = np.where(x % 4 < 2, 200, 50).astype(np.uint8)
    img = np.repeat(np.repeat(row[None, :, None], 97, 0), 3, 2)
    return img[:, 4:135].copy(), img[:, 3:134].copy(), img[:, 5:136].copy()


def test_ties():
    motion, diag, _ = _check(_stripes())
    assert diag[1].tolist() == [1, 35, 35, 35] and motion[1].tolist() == [1, 0, 1, 0] and motion[2].tolist() == [-2, 0, 1, 0]


def test_a_pan_beyond_the_reach_a_flat_frame_and_size_changes():
    """only equality is asserted for the pan of 40 px at a reach of 16"""
    k2 = motion_cases.recover_frames("k2", ((0, 0), (40, 0), (0, 0)))
    k1 = motion_cases.recover_frames("k1", PANS8)
    flat = np.full((192, 256, 3), 90, np.uint8)
    small = motion_cases.texture(3, 30, 30, 4)
    frames = [k2[0], k2[1], k2[2], flat, k2[0], k1[0], k1[1], small, small, k1[2], np.full((1, 700, 3), 7, np.uint8)]
    motion, diag, _ = _check(frames)
    assert motion[:, 2].tolist() == [0, motion[1, 2], 1, 1, 0, 0, 1, 0, 0, 0, 0]
    assert diag[7].tolist() == [1, 0, 0, 0] and diag[10].tolist() == [5, 0, 0, 0]


@pytest.mark.parametrize("settings", [dict(search=1), dict(search=16), dict(grid=32), dict(grid=32, search=1, min_blocks=1),
                                      dict(texture=60, min_blocks=30), dict(grid=100, search=5)],
                         ids=["search1", "search16", "grid32", "grid32_one_block", "texture", "grid100"])
def test_settings(settings):
    pans = ((0, 0), (2, 0), (-2, 2), (0, -2)) if settings.get("search") == 1 or settings.get("grid") == 32 else PANS8[:4]
    if settings.get("search") == 16:
        pans = ((0, 0), (31, 0), (-30, -32), (5, 29))
    motion, diag, _ = _check(motion_cases.recover_frames("k2", pans), settings=settings)
    if settings == dict(grid=32):
        assert diag[1].tolist() == [8, 0, 0, 0]
    if settings == dict(grid=32, search=1, min_blocks=1):
        assert diag[1].tolist() == [8, 1, 1, 1] and motion[1, 2] == 1
    if settings.get("search") == 16:
        assert np.abs(motion[1:, :2] - np.array(pans[1:], np.float32)).max() <= 1.0 and (motion[1:, 2] == 1).all()


def test_two_streams_in_one_launch():
    """two cameras of different sizes interleaved row by row; a stream without a row keeps its bytes"""
    a, b = motion_cases.recover_frames("k1", PANS8), motion_cases.recover_frames("k2", PANS8)
    frames = [f for pair in zip(a, b) for f in pair]
    streams = [2, 0] * 8
    want = _reference(frames, streams, None, 3)
    dev = Device(3)
    dev.state[1].fill_(SENTINEL_BYTE)
    motion, diag, raw = dev.run(frames, streams, None)
    assert np.array_equal(_bits(motion), _bits(want[0])) and np.array_equal(diag, want[1])
    assert np.array_equal(raw[0], want[2][0]) and np.array_equal(raw[2], want[2][2]) and (raw[1] == SENTINEL_BYTE).all()
    alone = _reference(a, [0] * 8, None, 1)
    assert np.array_equal(_bits(motion[0::2]), _bits(alone[0]))


def test_33_rows_are_split():
    from codetr import _cabi

    frames = (motion_cases.recover_frames("k1", PANS8) * 5)[:33]
    before = _cabi.CALLS["motion_estimate"]
    _check(frames)
    assert _cabi.CALLS["motion_estimate"] == before + 2


def test_chunking_does_not_matter():
    """the same frames as one launch, frame by frame and as 3 + 5: a stream's first row of a launch reads the state that
    its last row replaces"""
    frames = motion_cases.recover_frames("k2", PANS8)
    results = [_check(frames, chunks=chunks) for chunks in ([8], [1] * 8, [3, 5])]
    for motion, diag, raw in results[1:]:
        assert np.array_equal(_bits(motion), _bits(results[0][0])) and np.array_equal(diag, results[0][1])
        assert np.array_equal(raw, results[0][2])


def test_arguments():
    from codetr import hip_ops

    state = hip_ops.new_motion_state(1, DEV)
    buf = torch.zeros(30 * 30 * 3, dtype=torch.uint8, device=DEV)
    for bad in (dict(grid=31), dict(search=17), dict(search=0), dict(texture=-1), dict(min_blocks=0), dict(block=8)):
        with pytest.raises(ValueError):
            hip_ops.estimate_motion(buf, [(0, 30, 30)], state, settings=bad)
    with pytest.raises(ValueError):
        hip_ops.estimate_motion(buf, [(1, 30, 30)], state)               # outside the buffer
    with pytest.raises(ValueError):
        hip_ops.estimate_motion(buf, [(0, 30, 30)], state, streams=1)     # stream 1 of 1
    with pytest.raises(RuntimeError):
        hip_ops.estimate_motion(buf.cpu(), [(0, 30, 30)], state)         # the package computes on the GPU only
    assert not state.cpu().numpy().any()                                  # nothing was launched


# ---- 2. the tracker with a motion -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pan_motions():
    est = motion_ref.MotionRef()
    out = np.zeros((10, 4), np.float32)
    for f, img in enumerate(motion_cases.pan_frames()):
        out[f, :3] = est.estimate(img)[0]
    out.setflags(write=False)
    return out


def _dets(boxes, scores, labels, count, dtype):
    from codetr import hip_ops

    return hip_ops.Detections(torch.as_tensor(np.asarray(boxes)).to(dtype).to(DEV), torch.as_tensor(np.asarray(scores)).to(dtype).to(DEV),
                              torch.as_tensor(np.asarray(labels)).to(DEV), torch.as_tensor(np.asarray(count)).to(DEV), None)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_track_update_with_the_pan_sequence(association, dtype):
    from codetr import _cabi, hip_ops

    boxes, scores, labels, count = motion_cases.pan_boxes()
    motions = _pan_motions()
    dets = _dets(boxes, scores, labels, count, dtype)
    ref = (TrackMotionRef if association == "greedy" else TrackAssignMotionRef)()
    want = np.stack([ref.update(dets.boxes[f].cpu(), dets.scores[f].cpu(), labels[f], count[f], motion=motions[f])
                     for f in range(10)])
    assert (want == np.arange(1, 7)).all()
    state = hip_ops.new_track_state(1, 256, DEV)
    before = _cabi.CALLS["track_update3"]
    ids = hip_ops.track_update(dets, state, association=association, motion=torch.from_numpy(motions.copy()).to(DEV))
    assert _cabi.CALLS["track_update3"] == before + 1
    assert np.array_equal(ids.cpu().numpy(), want)
    _assert_state(hip_ops.track_state_to_host(state), 0, ref.state())
    # in two launches, and without the motion
    state2 = hip_ops.new_track_state(1, 256, DEV)
    m = torch.from_numpy(motions.copy()).to(DEV)
    parts = [hip_ops.track_update(hip_ops.Detections(*(t[a:b] for t in dets[:4]), None), state2, association=association,
                                  motion=m[a:b]) for a, b in ((0, 4), (4, 10))]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), want) and torch.equal(state2, state)
    plain = hip_ops.track_update(dets, hip_ops.new_track_state(1, 256, DEV), association=association).cpu().numpy()
    assert (plain[[3, 5, 6, 8]] < -6).all() and (plain[[0, 1, 2, 4, 7, 9]] == np.arange(1, 7)).all()


def test_track_update_large_lds():
    """max_tracks = 512, Q = 1024: the kernel needs the opt-in to large LDS"""
    from codetr import hip_ops

    b, s, l, c = track_cases.cached_sequence("dense")
    dets = _dets(b, s, l, c, torch.float32)
    motions = np.array([[0, 0, 0, 0], [3.5, -2.25, 1, 0], [-1.0, 0.5, 1, 0]], np.float32)
    ref = TrackMotionRef(dict(max_tracks=512))
    want = np.stack([ref.update(dets.boxes[f].cpu(), dets.scores[f].cpu(), l[f], c[f], motion=motions[f]) for f in range(3)])
    assert ref.log["A"] > 256 and ref.log["refused"] > 0
    state = hip_ops.new_track_state(1, 512, DEV)
    ids = hip_ops.track_update(dets, state, settings=dict(max_tracks=512), motion=torch.from_numpy(motions).to(DEV))
    assert np.array_equal(ids.cpu().numpy(), want)
    _assert_state(hip_ops.track_state_to_host(state), 0, ref.state())


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_motions_that_change_nothing(association):
    """all zero with valid 1, valid 0 with a garbage dx, valid 1 with a NaN dx (or an infinite dy): the ids and the state
    bytes of motion=None -- which calls the entry points it always did"""
    from codetr import _cabi, hip_ops

    b, s, l, c = track_cases.cached_sequence("reference")
    dets = _dets(b, s, l, c, torch.float16)
    N = len(c)
    before = dict(_cabi.CALLS)
    state = hip_ops.new_track_state(1, track_cases.SETTINGS["max_tracks"], DEV)
    want = hip_ops.track_update(dets, state, settings=track_cases.SETTINGS, association=association)
    key = "track_update" if association == "greedy" else "track_update2"
    assert _cabi.CALLS[key] == before[key] + 1 and _cabi.CALLS["track_update3"] == before["track_update3"]
    nan, inf = float("nan"), float("inf")
    for row in ([0, 0, 1, 0], [1e9, -3e5, 0, 0], [nan, 2, 1, 0], [2, inf, 1, 0], [5, 5, 2, 0], [nan, nan, 0, nan]):
        st = hip_ops.new_track_state(1, track_cases.SETTINGS["max_tracks"], DEV)
        motion = torch.tensor([row] * N, dtype=torch.float32, device=DEV)
        ids = hip_ops.track_update(dets, st, settings=track_cases.SETTINGS, association=association, motion=motion)
        assert torch.equal(ids, want) and torch.equal(st, state), row
    with pytest.raises(ValueError):
        hip_ops.track_update(dets, state, settings=track_cases.SETTINGS, motion=torch.zeros((N, 3), device=DEV))


# ---- 3. the Inferencer ------------------------------------------------------------------------------------------------
def _patched(frames):
    """the pan frames with their number k in a constant 8 x 8 corner patch (red = 8 k)"""
    out = []
    for k, f in enumerate(frames):
        f = f.copy()
        f[:8, :8] = (8 * k, 100, 50)
        out.append(f)
    return out


def _stub(inf, hw):
    """a scripted model: reads the frame number from the corner patch and returns the six boxes fixed in the scene (in
    the coordinates of the resized image), then two rows of clutter"""
    from codetr.inferencer import rescale_size

    mean, std = inf.mean[0], inf.std[0]
    nh, nw = rescale_size(hw[0], hw[1], inf.scale)
    shifts = torch.tensor(motion_cases.cumulative(motion_cases.PANS), dtype=torch.float32)
    origins = torch.tensor(motion_cases.BOX_ORIGINS + [(5, 5), (200, 150)], dtype=torch.float32)

    def model(x, m):
        N = x.shape[0]
        k = torch.round((x[:, 0, 0, 0].float() * std + mean) / 8).long().clamp(0, 9).cpu()
        xy = origins[None] + shifts[k][:, None]                                           # [N, 8, 2]
        boxes = torch.cat((xy, xy + torch.tensor([12.0, 24.0])), -1) * torch.tensor([nw / hw[1], nh / hw[0]] * 2)
        scores = torch.tensor([0.95, 0.94, 0.93, 0.92, 0.91, 0.90, 0.02, 0.02]).expand(N, 8)
        return boxes.to(x.device, x.dtype), scores.to(x.device, x.dtype).contiguous(), torch.zeros((N, 8), dtype=torch.long,
                                                                                                  device=x.device)
    return model


def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    inf = Inferencer(None, SWIN, dataset_meta=None, **kw)
    inf.model = _stub(inf, motion_cases.PAN_HW)
    return inf


def _reference_run(frames, preds):
    """motion_ref over the frames and track_motion_ref over the predictions the Inferencer returned"""
    est, ref, ids, motions = motion_ref.MotionRef(), TrackMotionRef(), [], []
    for img, p in zip(frames, preds):
        (dx, dy, valid), _ = est.estimate(img)
        n = len(p["labels"])
        ids.append(ref.update(np.asarray(p["bboxes"], np.float32).reshape(n, 4), np.asarray(p["scores"], np.float32),
                              np.asarray(p["labels"], np.int64), motion=(dx, dy, valid)).tolist())
        motions.append([float(dx), float(dy)] if valid == 1 else None)
    return ids, motions


def test_inferencer_keeps_the_ids_over_the_pan():
    from codetr import _cabi

    frames = _patched(motion_cases.pan_frames())
    inf = _inferencer(tracker={}, track_motion="translation")
    before = _cabi.CALLS["motion_estimate"]
    preds = inf(frames[:6], device=DEV, dtype=torch.float32, batch_size=4)["predictions"]      # chunks of 4 + 2, then 4
    preds += inf(frames[6:], device=DEV, dtype=torch.float32, batch_size=4)["predictions"]
    assert _cabi.CALLS["motion_estimate"] == before + 3
    want_ids, want_motion = _reference_run(frames, preds)
    assert [p["track_ids"] for p in preds] == want_ids
    assert [p["camera_motion"] for p in preds] == want_motion
    assert all(p["track_ids"][:6] == [1, 2, 3, 4, 5, 6] for p in preds)
    assert preds[0]["camera_motion"] is None and all(p["camera_motion"] is not None for p in preds[1:])
    for p, pan in zip(preds[1:], motion_cases.PANS[1:]):
        assert max(abs(p["camera_motion"][0] - pan[0]), abs(p["camera_motion"][1] - pan[1])) <= 0.5
    # frame by frame: the same
    single = _inferencer(tracker={}, track_motion=dict(type="translation"))(frames, device=DEV, dtype=torch.float32,
                                                                            batch_size=1)["predictions"]
    assert [(p["track_ids"], p["camera_motion"]) for p in single] == [(p["track_ids"], p["camera_motion"]) for p in preds]
    _same(single, preds)
    # without the motion: the ids are lost, no key, no launch
    before = _cabi.CALLS["motion_estimate"]
    plain = _inferencer(tracker={})(frames, device=DEV, dtype=torch.float32, batch_size=4)["predictions"]
    assert _cabi.CALLS["motion_estimate"] == before and all("camera_motion" not in p for p in plain)
    assert all(i < -6 for i in plain[3]["track_ids"][:6]) and plain[2]["track_ids"][:6] == [1, 2, 3, 4, 5, 6]
    _same(plain, preds)
    # reset_tracks: the stream's thumbnail goes with its tracks
    inf.reset_tracks(0)
    again = inf(frames[4:6], device=DEV, dtype=torch.float32, batch_size=2)["predictions"]
    assert again[0]["camera_motion"] is None and again[1]["camera_motion"] == preds[5]["camera_motion"]
    assert again[0]["track_ids"][:6] == [1, 2, 3, 4, 5, 6]


def test_inferencer_two_cameras_do_not_mix():
    frames = _patched(motion_cases.pan_frames())
    order = [0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7]             # camera 5: frames 0..5, camera 2: frames 2..7, interleaved
    inf = _inferencer(tracker={}, track_motion="translation")
    preds = inf([frames[k] for k in order], device=DEV, dtype=torch.float16, batch_size=4, streams=[5, 2] * 6)["predictions"]
    for cam in (0, 1):
        want_ids, want_motion = _reference_run([frames[k] for k in order[cam::2]], preds[cam::2])
        assert [p["track_ids"] for p in preds[cam::2]] == want_ids
        assert [p["camera_motion"] for p in preds[cam::2]] == want_motion
        assert all(p["track_ids"][:6] == [1, 2, 3, 4, 5, 6] for p in preds[cam::2])


def test_inferencer_estimates_before_it_draws():
    """with a visualizer the boxes are drawn into the buffer the estimate reads: the estimate comes first"""
    frames = _patched(motion_cases.pan_frames())[:6]
    kw = dict(tracker={}, track_motion="translation")
    plain = _inferencer(**kw)(frames, device=DEV, dtype=torch.float32, batch_size=3)["predictions"]
    inf = _inferencer(visualizer=dict(classes=["thing"], line_width=5), **kw)
    out = inf(frames, return_vis=True, pred_score_thr=0.3, device=DEV, dtype=torch.float32, batch_size=3)
    assert any(not np.array_equal(v, f) for v, f in zip(out["visualization"], frames))        # something was drawn
    assert [p["camera_motion"] for p in out["predictions"]] == [p["camera_motion"] for p in plain]
    assert [p["track_ids"] for p in out["predictions"]] == [p["track_ids"] for p in plain]


def test_inferencer_arguments():
    from codetr.inferencer import Inferencer

    with pytest.raises(ValueError):
        Inferencer(None, SWIN, dataset_meta=None, track_motion="translation")                   # no tracker
    for bad in ("affine", dict(grid=160), dict(type="translation", search=40), 3):
        with pytest.raises(ValueError):
            Inferencer(None, SWIN, dataset_meta=None, tracker={}, track_motion=bad)
    inf = Inferencer(None, SWIN, dataset_meta=None, tracker={}, track_motion=dict(type="translation", search=16, grid=64))
    assert inf.track_motion == dict(grid=64, search=16, texture=2, min_blocks=4)
