"""GPU: the similarity camera motion -- `codetr_motion_estimate2_u8` (csrc/motion.hip), `codetr_track_update4_*` and the
Inferencer's `track_motion="similarity"` -- against the numpy restatements (tests/motion_sim_ref.py,
tests/track_motion_sim_ref.py), bit for bit: the eight motion floats, the eight diag ints, the state bytes, the ids of every
row and the whole decoded track state.  The motion states sit between sentinel-filled guard rows."""
import functools

import numpy as np
import pytest
import torch

import motion_cases
import motion_ref
import motion_sim_cases as cases
import motion_sim_ref
import track_cases
from test_inferencer_batch_gpu import DEV, SWIN
from test_motion_gpu import SENTINEL_BYTE, _bits, _dets, _stripes
from test_track_gpu import _assert_state
from track_motion_sim_ref import TrackAssignMotionSimRef, TrackMotionSimRef

pytestmark = pytest.mark.gpu
SMALL = ((1.0, 0.0, (0, 0)), (1.0, 0.0, (2, 0)), (1.01, 0.004, (-2, 2)), (0.99, -0.004, (0, -2)))   # within a reach of one cell


def _reference(frames, streams, settings, S, models=None):
    """-> (motion [N, 8] float32, diag [N, 8] int32, states [S, bytes] uint8) of the restatement; models: per frame
    "similarity" (the default) or "translation" (its row is the four floats and ints of MotionRef, the rest zero)"""
    refs = [motion_sim_ref.MotionSimRef(settings) for _ in range(S)]
    motion, diag = np.zeros((len(frames), 8), np.float32), np.zeros((len(frames), 8), np.int32)
    for n, (img, s) in enumerate(zip(frames, streams)):
        if models is not None and models[n] == "translation":
            m, d = motion_ref.MotionRef.estimate(refs[s], img)
            motion[n, :3], diag[n, :4] = m, d
        else:
            motion[n], diag[n] = refs[s].estimate(img)
    return motion, diag, np.stack([r.state_bytes() for r in refs])


class Device:
    """S motion states between two guard rows; `run` feeds the frames in launches of `chunks` rows"""

    def __init__(self, S):
        from codetr import hip_ops

        self.all = hip_ops.new_motion_state(S + 2, DEV)
        self.all[0].fill_(SENTINEL_BYTE)
        self.all[-1].fill_(SENTINEL_BYTE)
        self.state = self.all[1:-1]

    def run(self, frames, streams, settings, chunks=None, models=None):
        from codetr import hip_ops

        motion, diag, at = [], [], 0
        for n in chunks or [len(frames)]:
            part = frames[at:at + n]
            offsets = np.cumsum([0] + [im.size for im in part]).tolist()
            buf = torch.from_numpy(np.concatenate([im.reshape(-1) for im in part])).to(DEV)
            rows = [(o, im.shape[0], im.shape[1]) for o, im in zip(offsets, part)]
            model = "similarity" if models is None else models[at]
            m, d = hip_ops.estimate_motion(buf, rows, self.state, streams[at:at + n], settings, model=model)
            m, d = m.cpu().numpy(), d.cpu().numpy()
            if model == "translation":
                m, d = np.pad(m, ((0, 0), (0, 4))), np.pad(d, ((0, 0), (0, 4)))
            motion.append(m)
            diag.append(d)
            at += n
        assert at == len(frames)
        raw = self.all.cpu().numpy()
        assert (raw[0] == SENTINEL_BYTE).all() and (raw[-1] == SENTINEL_BYTE).all()   # the guard rows
        return np.concatenate(motion), np.concatenate(diag), raw[1:-1]


def _check(frames, streams=None, settings=None, S=1, chunks=None, models=None):
    streams = streams or [0] * len(frames)
    want = _reference(frames, streams, settings, S, models)
    got = Device(S).run(list(frames), streams, settings, chunks, models)
    print("motion", got[0].tolist(), "diag", got[1].tolist())
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[1], want[1]), "diag"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), "motion"
    assert np.array_equal(got[2], want[2]), "state"
    return got


# ---- 1. the estimate --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k1", "k2", "sq"])
def test_three_sizes(name):
    """k = 1, k = 2 and the 81 blocks of 320 x 320 under zooms, rolls and pans, noise and a foreground that moves its own
    way; the bound on a and b is the CPU test's"""
    from test_motion_sim_cpu import BOUNDS

    motion, diag, _ = _check(cases.frames(name, cases.STEPS, True))
    assert (motion[1:, 3] == 2).all() and motion[0].tolist() == [0] * 8 and diag[0, 4:].tolist() == [0, 0, -1, -1]
    truth = np.array([cases.truth(s) for s in cases.STEPS[1:]])
    assert np.abs(motion[1:, 4:6] - truth).max() <= BOUNDS[name, True]
    assert diag[1, 1] == {"k1": 35, "k2": 35, "sq": 81}[name]


def test_one_row_of_collinear_blocks():
    motion, diag, _ = _check(cases.frames("row", cases.STEPS[:4]))
    assert (motion[1:, 3] == 2).all() and diag[1, :3].tolist() == [3, 5, 5]


@pytest.mark.parametrize("settings", [dict(search=1), dict(search=16), dict(grid=32), dict(grid=32, search=1, min_blocks=1),
                                      dict(min_blocks=1), dict(min_blocks=100), dict(texture=60, min_blocks=30)],
                         ids=["search1", "search16", "grid32", "grid32_one_block", "min1", "min100", "texture"])
def test_settings(settings):
    steps = SMALL if settings.get("search") == 1 or settings.get("grid") == 32 else cases.STEPS[:5]
    motion, diag, _ = _check(cases.frames("k2", steps), settings=settings)
    if settings == dict(grid=32):
        assert diag[1].tolist() == [8, 0, 0, 0, 0, 0, -1, -1]
    if settings == dict(grid=32, search=1, min_blocks=1):
        assert diag[1].tolist() == [8, 1, 1, 1, 0, 0, -1, -1] and motion[1, 2:].tolist() == [1, 1, 1, 0, 0, 0]   # the fallback
    if settings == dict(min_blocks=100):
        assert (motion[:, 2] == 0).all() and diag[1, 4] > 0 and diag[1, 5] > 0     # the search's figures are reported
    if settings in (dict(min_blocks=1), dict(search=16)):
        assert (motion[1:, 3] == 2).all()


def test_ties():
    """stripes: every block votes alike, every eligible pair has all 35 inliers and the lowest (i, j) wins: blocks 0 and 2"""
    motion, diag, _ = _check(_stripes())
    assert diag[1].tolist() == [1, 35, 35, 35, 489, 35, 0, 2] and diag[2, 4:].tolist() == [489, 35, 0, 2]
    assert motion[1].tolist() == [1, 0, 1, 2, 1, 0, 64, 48] and motion[2, :6].tolist() == [-2, 0, 1, 2, 1, 0]


def test_unrelated_frames_flat_frames_and_size_changes():
    """two frames of noise (only equality is asserted), a flat frame, a frame behind a flat one, size changes, no blocks"""
    rng = np.random.default_rng(5)
    noise = [rng.integers(0, 256, (192, 256, 3), dtype=np.uint8) for _ in range(2)]
    k2 = cases.frames("k2", cases.STEPS[:3])
    k1 = cases.frames("k1", cases.STEPS[:3])
    flat = np.full((192, 256, 3), 90, np.uint8)
    small = motion_cases.texture(3, 30, 30, 4)
    frames = [noise[0], noise[1], k2[0], k2[1], flat, k2[0], k1[0], k1[1], small, small, k1[2],
              np.full((1, 700, 3), 7, np.uint8)]
    motion, diag, _ = _check(frames)
    assert motion[3:, 3].tolist() == [2, 2, 0, 0, 2, 0, 0, 0, 0]
    assert diag[8].tolist() == [1, 0, 0, 0, 0, 0, -1, -1] and diag[11].tolist() == [5, 0, 0, 0, 0, 0, -1, -1]


def test_two_streams_in_one_launch():
    """two cameras of different sizes interleaved row by row; a stream without a row keeps its bytes"""
    a, b = cases.frames("k1", cases.STEPS[:6], True), cases.frames("k2", cases.STEPS[:6], True)
    frames = [f for pair in zip(a, b) for f in pair]
    streams = [2, 0] * 6
    want = _reference(frames, streams, None, 3)
    dev = Device(3)
    dev.state[1].fill_(SENTINEL_BYTE)
    motion, diag, raw = dev.run(frames, streams, None)
    assert np.array_equal(_bits(motion), _bits(want[0])) and np.array_equal(diag, want[1])
    assert np.array_equal(raw[0], want[2][0]) and np.array_equal(raw[2], want[2][2]) and (raw[1] == SENTINEL_BYTE).all()
    alone = _reference(a, [0] * 6, None, 1)
    assert np.array_equal(_bits(motion[0::2]), _bits(alone[0]))


def test_33_rows_are_split():
    from codetr import _cabi

    frames = (cases.frames("k1", cases.STEPS[:6]) * 6)[:33]
    before = dict(_cabi.CALLS)
    _check(frames)
    assert _cabi.CALLS["motion_estimate2"] == before["motion_estimate2"] + 2
    assert _cabi.CALLS["motion_estimate"] == before["motion_estimate"]


def test_chunking_does_not_matter():
    frames = cases.frames("k2", cases.STEPS[:8], True)
    results = [_check(frames, chunks=chunks) for chunks in ([8], [1] * 8, [3, 5])]
    for motion, diag, raw in results[1:]:
        assert np.array_equal(_bits(motion), _bits(results[0][0])) and np.array_equal(diag, results[0][1])
        assert np.array_equal(raw, results[0][2])


def test_a_stream_alternates_between_the_two_entry_points():
    """the state is one: each call's predecessor is the thumbnail the other entry point left"""
    from codetr import _cabi

    frames = cases.frames("k2", cases.STEPS[:8])
    chunks = [1, 1, 2, 1, 1, 2]
    models = ["similarity", "translation", "similarity", "similarity", "translation", "translation", "similarity", "similarity"]
    before = dict(_cabi.CALLS)
    motion, _, _ = _check(frames, chunks=chunks, models=models)
    assert _cabi.CALLS["motion_estimate2"] == before["motion_estimate2"] + 3
    assert _cabi.CALLS["motion_estimate"] == before["motion_estimate"] + 3
    assert motion[1:, 2].tolist() == [0, 1, 1, 0, 0, 1, 1]       # a translation is invalid under these zooms and rolls


def test_arguments():
    from codetr import _motion, hip_ops

    state = hip_ops.new_motion_state(1, DEV)
    buf = torch.zeros(30 * 30 * 3, dtype=torch.uint8, device=DEV)
    for bad in (dict(grid=31), dict(search=17), dict(search=0), dict(texture=-1), dict(min_blocks=0), dict(min_blocks=101)):
        with pytest.raises(ValueError):
            hip_ops.estimate_motion(buf, [(0, 30, 30)], state, settings=bad, model="similarity")
    for bad in ("affine", None, 2):
        with pytest.raises(ValueError):
            hip_ops.estimate_motion(buf, [(0, 30, 30)], state, model=bad)
    with pytest.raises(ValueError):
        hip_ops.estimate_motion(buf, [(1, 30, 30)], state, model="similarity")               # outside the buffer
    with pytest.raises(ValueError):
        hip_ops.estimate_motion(buf, [(0, 30, 30)], state, streams=1, model="similarity")     # stream 1 of 1
    # the entry point's own checks: a scratch of the translation form's size, a setting out of range, a row past the buffer
    motion = torch.full((1, 8), 7.0, device=DEV)
    diag = torch.full((1, 8), 7, dtype=torch.int32, device=DEV)
    assert _motion.work2_bytes(1) > _motion.work_bytes(1) and _motion.work2_bytes(0) < 0 and _motion.work2_bytes(33) < 0
    small = torch.empty(_motion.work_bytes(1), dtype=torch.uint8, device=DEV)
    work = torch.empty(_motion.work2_bytes(1), dtype=torch.uint8, device=DEV)
    for args in ((buf, [(0, 30, 30)], [0], state, (160, 8, 2, 4), small), (buf, [(0, 30, 30)], [0], state, (160, 8, 2, 101), work),
                 (buf, [(0, 31, 30)], [0], state, (160, 8, 2, 4), work), (buf, [(0, 30, 30)], [1], state, (160, 8, 2, 4), work)):
        with pytest.raises(RuntimeError):
            _motion.estimate(*args, motion, diag, similarity=True)
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and (motion == 7).all() and (diag == 7).all()   # nothing was launched


# ---- 2. the tracker with a similarity ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _box_motions():
    est = motion_sim_ref.MotionSimRef()
    out = np.stack([np.array(est.estimate(img)[0], np.float32) for img in cases.box_frames()])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_track_update_with_the_eight_boxes(association, dtype):
    from codetr import _cabi, hip_ops

    boxes, scores, labels, count = cases.scene_boxes()
    motions = _box_motions()
    assert (motions[1:, 3] == 2).all()
    dets = _dets(boxes, scores, labels, count, dtype)
    ref = (TrackMotionSimRef if association == "greedy" else TrackAssignMotionSimRef)()
    want = np.stack([ref.update(dets.boxes[f].cpu(), dets.scores[f].cpu(), labels[f], count[f], motion=motions[f])
                     for f in range(10)])
    assert (want == np.arange(1, 9)).all()
    state = hip_ops.new_track_state(1, 256, DEV)
    before = dict(_cabi.CALLS)
    ids = hip_ops.track_update(dets, state, association=association, motion=torch.from_numpy(motions.copy()).to(DEV))
    assert _cabi.CALLS["track_update4"] == before["track_update4"] + 1 and _cabi.CALLS["track_update3"] == before["track_update3"]
    assert np.array_equal(ids.cpu().numpy(), want)
    _assert_state(hip_ops.track_state_to_host(state), 0, ref.state())
    # in two launches, and without the motion
    state2 = hip_ops.new_track_state(1, 256, DEV)
    m = torch.from_numpy(motions.copy()).to(DEV)
    parts = [hip_ops.track_update(hip_ops.Detections(*(t[a:b] for t in dets[:4]), None), state2, association=association,
                                  motion=m[a:b]) for a, b in ((0, 4), (4, 10))]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), want) and torch.equal(state2, state)
    plain = hip_ops.track_update(dets, hip_ops.new_track_state(1, 256, DEV), association=association).cpu().numpy()
    assert int(np.abs(plain).max()) > 8


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_rows_of_the_other_models(association):
    """model 1 rows: codetr_track_update3_*'s ids and state bytes with the same dx, dy; NULL, model 0, another model and
    non-finite rows: those of motion=None"""
    from codetr import hip_ops

    b, s, l, c = track_cases.cached_sequence("reference")
    dets = _dets(b, s, l, c, torch.float16)
    N = len(c)
    T = track_cases.SETTINGS["max_tracks"]
    kw = dict(settings=track_cases.SETTINGS, association=association)

    def run(motion):
        st = hip_ops.new_track_state(1, T, DEV)
        m = None if motion is None else torch.tensor(motion, dtype=torch.float32, device=DEV)
        return hip_ops.track_update(dets, st, motion=m, **kw), st

    shifts = [[3.5 * (-1) ** f, -2.25 + f % 3, 1, 0] for f in range(N)]
    want_ids, want_state = run(shifts)                                              # update3
    got_ids, got_state = run([r[:3] + [1, 0.5, 0.5, 100, 100] for r in shifts])       # model 1: a, b, px, py are not read
    assert torch.equal(got_ids, want_ids) and torch.equal(got_state, want_state)
    assert not torch.equal(want_state, run(None)[1])                                # (the shifts do change the state)
    none_ids, none_state = run(None)
    nan, inf = float("nan"), float("inf")
    for row in ([3, 4, 1, 0, 1.1, 0.1, 50, 50], [3, 4, 1, 3, 1.1, 0.1, 50, 50], [nan, 4, 1, 1, 1, 0, 0, 0],
                [3, inf, 1, 1, 1, 0, 0, 0], [3, 4, 1, 2, nan, 0.1, 50, 50], [3, 4, 1, 2, 1.1, inf, 50, 50],
                [3, 4, 1, 2, 1.1, 0.1, nan, 50], [3, 4, 1, 2, 1.1, 0.1, 50, -inf], [nan, 4, 1, 2, 1.1, 0.1, 50, 50],
                [3, 4, 0, 0, 0, 0, 0, 0]):
        ids, st = run([row] * N)
        assert torch.equal(ids, none_ids) and torch.equal(st, none_state), row
    with pytest.raises(ValueError):
        hip_ops.track_update(dets, none_state, motion=torch.zeros((N, 6), device=DEV), **kw)


def test_track_update_large_lds():
    """max_tracks = 512, Q = 1024: the kernel needs the opt-in to large LDS"""
    from codetr import hip_ops

    b, s, l, c = track_cases.cached_sequence("dense")
    dets = _dets(b, s, l, c, torch.float32)
    motions = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [3.5, -2.25, 1, 2, 1.03125, -0.015625, 400, 300],
                        [-1.0, 0.5, 1, 1, 1, 0, 0, 0]], np.float32)
    ref = TrackMotionSimRef(dict(max_tracks=512))
    want = np.stack([ref.update(dets.boxes[f].cpu(), dets.scores[f].cpu(), l[f], c[f], motion=motions[f]) for f in range(3)])
    assert ref.log["A"] > 256 and ref.log["refused"] > 0
    state = hip_ops.new_track_state(1, 512, DEV)
    ids = hip_ops.track_update(dets, state, settings=dict(max_tracks=512), motion=torch.from_numpy(motions).to(DEV))
    assert np.array_equal(ids.cpu().numpy(), want)
    _assert_state(hip_ops.track_state_to_host(state), 0, ref.state())


# ---- 3. the Inferencer ------------------------------------------------------------------------------------------------
def _patched(frames):
    """the frames with their number k in a constant 8 x 8 corner patch (red = 8 k)"""
    out = []
    for k, f in enumerate(frames):
        f = f.copy()
        f[:8, :8] = (8 * k, 100, 50)
        out.append(f)
    return out


def _stub(inf, hw):
    """a scripted model: reads the frame number from the corner patch and returns the eight boxes fixed in the scene (in
    the coordinates of the resized image), then two rows of clutter"""
    from codetr.inferencer import rescale_size

    mean, std = inf.mean[0], inf.std[0]
    nh, nw = rescale_size(hw[0], hw[1], inf.scale)
    table = torch.from_numpy(cases.scene_boxes()[0])                                         # [10, 8, 4]
    clutter = torch.tensor([[5.0, 5.0, 17.0, 29.0], [200.0, 150.0, 212.0, 174.0]])

    def model(x, m):
        N = x.shape[0]
        k = torch.round((x[:, 0, 0, 0].float() * std + mean) / 8).long().clamp(0, 9).cpu()
        boxes = torch.cat((table[k], clutter[None].expand(N, 2, 4)), 1) * torch.tensor([nw / hw[1], nh / hw[0]] * 2)
        scores = torch.tensor([0.95, 0.94, 0.93, 0.92, 0.91, 0.90, 0.89, 0.88, 0.02, 0.02]).expand(N, 10)
        return boxes.to(x.device, x.dtype), scores.to(x.device, x.dtype).contiguous(), torch.zeros((N, 10), dtype=torch.long,
                                                                                                   device=x.device)
    return model


def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    inf = Inferencer(None, SWIN, dataset_meta=None, **kw)
    inf.model = _stub(inf, cases.BOX_HW)
    return inf


def _reference_run(frames, preds):
    """motion_sim_ref over the frames and track_motion_sim_ref over the predictions the Inferencer returned"""
    est, ref, ids, motions, transforms = motion_sim_ref.MotionSimRef(), TrackMotionSimRef(), [], [], []
    for img, p in zip(frames, preds):
        m, _ = est.estimate(img)
        n = len(p["labels"])
        ids.append(ref.update(np.asarray(p["bboxes"], np.float32).reshape(n, 4), np.asarray(p["scores"], np.float32),
                              np.asarray(p["labels"], np.int64), motion=m).tolist())
        motions.append([float(m[0]), float(m[1])] if m[2] == 1 else None)
        transforms.append(motion_sim_ref.transform(m))
    return ids, motions, transforms


def test_inferencer_keeps_the_ids_over_zoom_and_roll():
    from codetr import _cabi

    frames = _patched(cases.box_frames())
    inf = _inferencer(tracker={}, track_motion="similarity")
    before = dict(_cabi.CALLS)
    preds = inf(frames[:6], device=DEV, dtype=torch.float32, batch_size=4)["predictions"]      # chunks of 4 + 2, then 4
    preds += inf(frames[6:], device=DEV, dtype=torch.float32, batch_size=4)["predictions"]
    assert _cabi.CALLS["motion_estimate2"] == before["motion_estimate2"] + 3
    assert _cabi.CALLS["track_update4"] == before["track_update4"] + 3
    assert _cabi.CALLS["motion_estimate"] == before["motion_estimate"] and _cabi.CALLS["track_update3"] == before["track_update3"]
    want_ids, want_motion, want_transform = _reference_run(frames, preds)
    assert [p["track_ids"] for p in preds] == want_ids
    assert [p["camera_motion"] for p in preds] == want_motion
    assert [p["camera_transform"] for p in preds] == want_transform
    assert all(p["track_ids"][:8] == [1, 2, 3, 4, 5, 6, 7, 8] for p in preds)
    assert preds[0]["camera_transform"] is None and preds[0]["camera_motion"] is None
    for p, step in zip(preds[1:], cases.STEPS[1:]):
        a, b = cases.truth(step)
        (m00, m01, _), (m10, m11, _) = p["camera_transform"]
        assert m00 == m11 and m01 == -m10 and abs(m00 - a) <= 0.004 and abs(m10 - b) <= 0.004   # the CPU test's sq bound
    # translation and none lose the ids; "translation" has no camera_transform key
    for kw in (dict(track_motion="translation"), dict()):
        other = _inferencer(tracker={}, **kw)(frames, device=DEV, dtype=torch.float32, batch_size=4)["predictions"]
        assert max(abs(i) for p in other for i in p["track_ids"]) > 8 and all("camera_transform" not in p for p in other)


def test_inferencer_two_cameras_do_not_mix():
    frames = _patched(cases.box_frames())
    order = [0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7]             # camera 5: frames 0..5, camera 2: frames 2..7, interleaved
    inf = _inferencer(tracker={}, track_motion=dict(type="similarity"))
    preds = inf([frames[k] for k in order], device=DEV, dtype=torch.float16, batch_size=4, streams=[5, 2] * 6)["predictions"]
    for cam in (0, 1):
        want_ids, want_motion, want_transform = _reference_run([frames[k] for k in order[cam::2]], preds[cam::2])
        assert [p["track_ids"] for p in preds[cam::2]] == want_ids
        assert [p["camera_transform"] for p in preds[cam::2]] == want_transform
        assert all(p["track_ids"][:8] == [1, 2, 3, 4, 5, 6, 7, 8] for p in preds[cam::2])


def test_inferencer_arguments():
    from codetr.inferencer import Inferencer

    with pytest.raises(ValueError):
        Inferencer(None, SWIN, dataset_meta=None, track_motion="similarity")                     # no tracker
    for bad in ("affine", dict(type="similarity", search=40), dict(type="similarity", block=8), dict(type="homography")):
        with pytest.raises(ValueError):
            Inferencer(None, SWIN, dataset_meta=None, tracker={}, track_motion=bad)
    inf = Inferencer(None, SWIN, dataset_meta=None, tracker={}, track_motion=dict(type="similarity", search=16, grid=64))
    assert inf.track_motion == dict(grid=64, search=16, texture=2, min_blocks=4) and inf.track_motion_model == "similarity"
    inf = Inferencer(None, SWIN, dataset_meta=None, tracker={}, track_motion="translation")
    assert inf.track_motion_model == "translation"
    assert Inferencer(None, SWIN, dataset_meta=None, tracker={}).track_motion_model is None


def test_inferencer_estimates_before_it_draws():
    """with a visualizer the boxes are drawn into the buffer the estimate reads: the estimate comes first"""
    frames = _patched(cases.box_frames())[:6]
    kw = dict(tracker={}, track_motion="similarity")
    plain = _inferencer(**kw)(frames, device=DEV, dtype=torch.float32, batch_size=3)["predictions"]
    inf = _inferencer(visualizer=dict(classes=["thing"], line_width=5), **kw)
    out = inf(frames, return_vis=True, pred_score_thr=0.3, device=DEV, dtype=torch.float32, batch_size=3)
    assert any(not np.array_equal(v, f) for v, f in zip(out["visualization"], frames))        # something was drawn
    assert [p["camera_transform"] for p in out["predictions"]] == [p["camera_transform"] for p in plain]
    assert [p["track_ids"] for p in out["predictions"]] == [p["track_ids"] for p in plain]
