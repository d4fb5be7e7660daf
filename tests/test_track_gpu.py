"""GPU: `codetr_track_update_*` and the Inferencer's tracker against `track_ref`, bit for bit -- the ids of every row and
the whole decoded state.  Id buffers are sentinel-filled and the states sit between sentinel-filled guard rows."""
import numpy as np
import pytest
import torch

import track_cases
from test_inferencer_batch_gpu import DEV, SWIN, _same
from track_ref import TrackRef

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
SENTINEL_ID, SENTINEL_BYTE = 0x5A5A5A5A, 0xA5


def _rounded(name, dtype):
    """a scripted sequence rounded once to `dtype`: (boxes, scores) tensors on the host, labels, count"""
    b, s, l, c = track_cases.cached_sequence(name)
    return torch.tensor(b).to(dtype), torch.tensor(s).to(dtype), l, c


def _thresholds(cfg):
    return (cfg["obj_score_thrs"]["high"], cfg["obj_score_thrs"]["low"], cfg["init_track_thr"],
            cfg["match_iou_thrs"]["high"], cfg["match_iou_thrs"]["low"], cfg["match_iou_thrs"]["tentative"])


class Device:
    """S stream states between two guard rows, and launches of codetr_track_update_* on sentinel-filled id buffers"""

    def __init__(self, S, settings):
        from codetr import hip_ops

        self.cfg = hip_ops.track_settings(settings)
        self.T = self.cfg["max_tracks"]
        self.all = hip_ops.new_track_state(S + 2, self.T, DEV)
        self.all[0].fill_(SENTINEL_BYTE)
        self.all[-1].fill_(SENTINEL_BYTE)
        self.state = self.all[1:-1]

    def launch(self, boxes, scores, labels, count, streams):
        """rows (frames) [N, Q, ..] on the host -> ids [N, Q] numpy"""
        from codetr import _cabi

        N, Q = scores.shape
        ids = torch.full((N + 2, Q), SENTINEL_ID, dtype=torch.int32, device=DEV)
        before = _cabi.CALLS["track_update"]
        _cabi.track_update(boxes.to(DEV).contiguous(), scores.to(DEV).contiguous(),
                           torch.as_tensor(labels).to(DEV).contiguous(), torch.as_tensor(count).to(DEV).contiguous(),
                           streams, self.state, self.T, _thresholds(self.cfg), self.cfg["num_frames_retain"],
                           self.cfg["num_tentatives"], self.cfg["weight_iou_with_det_scores"], ids[1:-1])
        assert _cabi.CALLS["track_update"] == before + 1
        torch.cuda.synchronize()
        host = ids.cpu().numpy()
        assert (host[0] == SENTINEL_ID).all() and (host[-1] == SENTINEL_ID).all()   # nothing outside [N, Q]
        assert (host[1:-1] != SENTINEL_ID).all()                                   # every element written
        return host[1:-1]

    def run(self, seq, chunks, stream=0):
        boxes, scores, labels, count = seq
        out, f = [], 0
        for n in chunks:
            out.append(self.launch(boxes[f:f + n], scores[f:f + n], labels[f:f + n], count[f:f + n], [stream] * n))
            f += n
        assert f == len(count)
        return np.concatenate(out)

    def decoded(self):
        from codetr import hip_ops

        raw = self.all.cpu().numpy()
        assert (raw[0] == SENTINEL_BYTE).all() and (raw[-1] == SENTINEL_BYTE).all()   # the guard rows
        return hip_ops.track_state_to_host(self.state)


def _assert_state(got, s, want):
    """stream s of a decoded device state == a track_ref State, every field bit for bit"""
    assert (got.f[s], got.next_id[s], got.refused[s]) == (want.f, want.next_id, want.refused)
    for name in ("id", "label", "hits", "tentative", "last"):
        assert np.array_equal(getattr(got, name)[s], getattr(want, name)), name
    for name in ("mean", "cov"):
        g, w = getattr(got, name)[s], getattr(want, name)
        assert g.dtype == w.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)), name


def _assert_rows_beyond_count_are_zero(ids, count):
    for f, c in enumerate(count):
        assert not ids[f, c:].any()


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_sequence(dtype):
    seq = _rounded("reference", dtype)
    want_ids, want_state, log = track_cases.run_reference(*seq, track_cases.SETTINGS)
    track_cases.assert_exercises_every_branch(log)   # on the reference alone, before the kernel is asked anything
    dev = Device(1, track_cases.SETTINGS)
    ids = dev.run(seq, [12])
    assert np.array_equal(ids, want_ids)
    _assert_rows_beyond_count_are_zero(ids, seq[3])
    _assert_state(dev.decoded(), 0, want_state)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_chunking_does_not_matter(dtype):
    """12 frames in one launch, in 12 launches and as 5 + 7: the frames of a stream are walked in order inside a launch"""
    seq = _rounded("reference", dtype)
    want_ids, want_state, _ = track_cases.run_reference(*seq, track_cases.SETTINGS)
    results = []
    for chunks in ([12], [1] * 12, [5, 7]):
        dev = Device(1, track_cases.SETTINGS)
        ids = dev.run(seq, chunks)
        dev.decoded()
        results.append((ids, dev.state.cpu().numpy()))
    for ids, raw in results:
        assert np.array_equal(ids, want_ids)
        assert np.array_equal(raw, results[0][1])          # the final state, byte for byte
    dev = Device(1, track_cases.SETTINGS)
    dev.run(seq, [12])
    _assert_state(dev.decoded(), 0, want_state)


def test_streams_are_independent():
    """two sequences interleaved row by row in one launch equal each alone; a stream without a row keeps its bytes"""
    from codetr import hip_ops

    dtype = torch.float16
    a, b = _rounded("reference", dtype), _rounded("second", dtype)
    want = [track_cases.run_reference(*s, track_cases.SETTINGS) for s in (a, b)]
    boxes, scores = torch.stack((a[0], b[0]), 1).flatten(0, 1), torch.stack((a[1], b[1]), 1).flatten(0, 1)
    labels, count = np.stack((a[2], b[2]), 1).reshape(24, -1), np.stack((a[3], b[3]), 1).reshape(24)
    dev = Device(3, track_cases.SETTINGS)
    dev.state[1].fill_(SENTINEL_BYTE)                       # stream 1 has no row in this launch
    ids = dev.launch(boxes, scores, labels, count, [2, 0] * 12)
    assert np.array_equal(ids[0::2], want[0][0]) and np.array_equal(ids[1::2], want[1][0])
    got = dev.decoded()
    _assert_state(got, 2, want[0][1])
    _assert_state(got, 0, want[1][1])
    assert (dev.state[1].cpu().numpy() == SENTINEL_BYTE).all()
    # the same through hip_ops.track_update, which splits more than 32 rows into launches: 2 x 12 + 12 rows of a third run
    state = hip_ops.new_track_state(3, track_cases.SETTINGS["max_tracks"], DEV)
    dets = hip_ops.Detections(torch.cat((boxes, a[0])).to(DEV), torch.cat((scores, a[1])).to(DEV),
                              torch.as_tensor(np.concatenate((labels, a[2]))).to(DEV),
                              torch.as_tensor(np.concatenate((count, a[3]))).to(DEV), None)
    ids = hip_ops.track_update(dets, state, [2, 0] * 12 + [1] * 12, track_cases.SETTINGS).cpu().numpy()
    assert np.array_equal(ids[0:24:2], want[0][0]) and np.array_equal(ids[1:24:2], want[1][0])
    assert np.array_equal(ids[24:], want[0][0])
    got = hip_ops.track_state_to_host(state)
    _assert_state(got, 1, want[0][1])
    _assert_state(got, 2, want[0][1])
    with pytest.raises(ValueError):
        hip_ops.track_update(dets, state, 3, track_cases.SETTINGS)         # stream 3 of 3
    with pytest.raises(ValueError):
        hip_ops.track_update(dets, state, 0, dict(max_tracks=21))          # not the state's


def test_limits_large():
    """Q = 1024 candidates (more than the workgroup's threads), 512 tracks (more than a wave, two per thread), more than
    512 starts on frame 0: the slots run out"""
    b, s, l, c = track_cases.cached_sequence("dense")
    seq = (torch.tensor(b).float(), torch.tensor(s).float(), l, c)
    settings = dict(max_tracks=512)
    want_ids, want_state, log = track_cases.run_reference(*seq, settings)
    assert int((seq[1][0] > 0.7).sum()) > 512 and log["refused"] > 0 and log["A"] > 256 and log["C"] > 0
    dev = Device(1, settings)
    ids = dev.run(seq, [3])
    assert np.array_equal(ids, want_ids)
    _assert_state(dev.decoded(), 0, want_state)


@pytest.mark.parametrize("Q", [985, 1000])
def test_around_the_64_kb_lds_threshold(Q):
    """the default 256 slots with Q near 1000: the kernel's LDS is 65 424 bytes at Q = 985 -- under 64 KB on its own, over
    it with what the compiler adds -- and 65 920 at Q = 1000; both sides of the opt-in to large LDS must launch"""
    b, s, l, c = track_cases.dense_sequence(frames=2, Q=Q)
    seq = (torch.tensor(b).float(), torch.tensor(s).float(), l, c)
    want_ids, want_state, log = track_cases.run_reference(*seq, dict(max_tracks=256))
    assert log["refused"] > 0 and log["A"] > 128
    dev = Device(1, dict(max_tracks=256))
    assert np.array_equal(dev.run(seq, [2]), want_ids)
    _assert_state(dev.decoded(), 0, want_state)


def test_limits_small():
    """Q = 1, one slot: the box is tracked; a second object is refused while the slot is held (frame 2) and takes it in
    the frame that retires the first (frame 3: f - last = 2), tentative until its third match"""
    settings = dict(max_tracks=1, num_frames_retain=2)
    A, B = (100.0, 100.0, 140.0, 180.0), (300.0, 300.0, 340.0, 380.0)
    rows = [A, A, B, B, B, B, B]
    seq = (torch.tensor(rows).view(7, 1, 4), torch.full((7, 1), 0.9), np.zeros((7, 1), np.int64), np.ones(7, np.int32))
    want_ids, want_state, log = track_cases.run_reference(*seq, settings)
    assert want_ids[:, 0].tolist() == [1, 1, 0, -2, -2, 2, 2] and log["refused"] == 1 and log["retired"] == 1
    dev = Device(1, settings)
    assert np.array_equal(dev.run(seq, [3, 4]), want_ids)
    _assert_state(dev.decoded(), 0, want_state)


def test_plain_iou_as_the_match_value():
    settings = dict(track_cases.SETTINGS, weight_iou_with_det_scores=False)
    seq = _rounded("reference", torch.float32)
    want_ids, want_state, _ = track_cases.run_reference(*seq, settings)
    dev = Device(1, settings)
    assert np.array_equal(dev.run(seq, [12]), want_ids)
    _assert_state(dev.decoded(), 0, want_state)


# ---- 2. the Inferencer ---------------------------------------------------------------------------------------------------
OBJECTS = 10


def _stub(inf, Q=16):
    """a scripted model: the frame number k sits in the red channel of the (constant) image, 8 k; object i moves by a
    fixed step per frame, is faint on some frames and absent on others; the last rows are low-score clutter"""
    mean, std = inf.mean[0], inf.std[0]

    def model(x, m):
        N, (H, W) = x.shape[0], x.shape[2:]
        k = torch.round((x[:, 0, 0, 0].float() * std + mean) / 8)[:, None]              # [N, 1]
        i = torch.arange(Q, device=x.device, dtype=torch.float32)[None]                  # [1, Q]
        cx = (0.06 + 0.11 * (i % 8) + 0.004 * k * (1 + i % 3)) * W
        cy = (0.2 + 0.4 * (i // 8) + 0.004 * k) * H
        w, h = (0.05 + 0.004 * (i % 4)) * W + 0 * k, (0.12 + 0.01 * (i % 3)) * H + 0 * k
        scores = 0.95 - 0.01 * i + 0 * k
        scores = torch.where((i + k) % 7 == 3, torch.full_like(scores, 0.3), scores)     # faint
        scores = torch.where((i + 2 * k) % 11 == 5, torch.full_like(scores, 0.02), scores)   # absent
        scores = torch.where(i >= OBJECTS, 0.15 + 0 * scores, scores)
        labels = (i % 3).long().expand(N, Q)
        boxes = torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), -1)
        return boxes.to(x.dtype), scores.to(x.dtype), labels.contiguous()
    return model


def _frames(ks, hw=(120, 160)):
    return [np.full(hw + (3,), (8 * k, 100, 50), np.uint8) for k in ks]


def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    inf = Inferencer(None, SWIN, dataset_meta=None, **kw)
    inf.model = _stub(inf)
    return inf


def _reference_ids(preds, settings=None):
    """track_ref over the predictions the Inferencer returned (the values a result dict holds are exact)"""
    ref, out = TrackRef(settings), []
    for p in preds:
        n = len(p["labels"])
        ids = ref.update(np.asarray(p["bboxes"], np.float32).reshape(n, 4), np.asarray(p["scores"], np.float32),
                         np.asarray(p["labels"], np.int64))
        out.append(ids.tolist())
    return out, ref


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_inferencer_plain_path(dtype):
    from codetr import _cabi

    frames = _frames(range(8))
    # batch_size 4 over two calls (chunks of 4 + 1, then 3), and frame by frame
    inf = _inferencer(tracker={})
    before = _cabi.CALLS["track_update"]
    preds = inf(frames[:5], device=DEV, dtype=dtype, batch_size=4)["predictions"]
    assert _cabi.CALLS["track_update"] == before + 2              # one launch per chunk
    preds += inf(frames[5:], device=DEV, dtype=dtype, batch_size=4)["predictions"]
    assert _cabi.CALLS["track_update"] == before + 3
    want, ref = _reference_ids(preds)
    assert [p["track_ids"] for p in preds] == want
    assert ref.log["A"] > 20 and ref.log["C"] > 0 and ref.log["started"] > OBJECTS - 2 and ref.state().next_id > 5
    assert all(len(p["track_ids"]) == len(p["labels"]) == len(p["scores"]) for p in preds)
    single = _inferencer(tracker={})(frames, device=DEV, dtype=dtype, batch_size=1)["predictions"]
    assert [p["track_ids"] for p in single] == want
    _same(single, preds)
    # no tracker: no key, no launch, the same predictions
    before = _cabi.CALLS["track_update"]
    plain = _inferencer()(frames, device=DEV, dtype=dtype, batch_size=4)["predictions"]
    assert _cabi.CALLS["track_update"] == before and all(set(p) == {"labels", "scores", "bboxes"} for p in plain)
    _same(plain, preds)
    # reset_tracks: the ids start at 1 again
    again = inf(frames[:2], device=DEV, dtype=dtype, batch_size=2)["predictions"]
    assert min(again[0]["track_ids"]) < 0     # the stream goes on: what frame 0 shows and no track is near starts tentative
    inf.reset_tracks()
    again = inf(frames[:2], device=DEV, dtype=dtype, batch_size=2)["predictions"]
    assert [p["track_ids"] for p in again] == want[:2] and again[0]["track_ids"][0] == 1


def test_inferencer_streams_are_two_cameras():
    ks = [0, 3, 1, 4, 2, 5, 3, 6, 4, 7]                      # camera 5: frames 0..4, camera 2: frames 3..7, interleaved
    inf = _inferencer(tracker=dict(num_tentatives=2))
    preds = inf(_frames(ks), device=DEV, dtype=torch.float16, batch_size=4, streams=[5, 2] * 5)["predictions"]
    for cam in (0, 1):
        want, _ = _reference_ids(preds[cam::2], dict(num_tentatives=2))
        assert [p["track_ids"] for p in preds[cam::2]] == want
        assert want[0][0] == 1                               # each camera counts from 1
    inf.reset_tracks(2)                                      # camera 2 forgets, camera 5 goes on
    more = inf(_frames([5, 8]), device=DEV, dtype=torch.float16, batch_size=2, streams=[5, 2])["predictions"]
    want5, _ = _reference_ids(preds[0::2] + more[:1], dict(num_tentatives=2))
    assert more[0]["track_ids"] == want5[-1]
    assert more[1]["track_ids"] == _reference_ids(more[1:], dict(num_tentatives=2))[0][0]


@pytest.mark.parametrize("kw", [dict(nms_type="config"), dict(slicing=dict(tile=(96, 96), overlap=0.25))],
                         ids=["soft_nms", "sliced"])
def test_inferencer_other_paths(kw):
    from codetr import _cabi

    inf = _inferencer(tracker={}, **kw)
    before = _cabi.CALLS["track_update"]
    preds = inf(_frames(range(6)), device=DEV, dtype=torch.float16, batch_size=3)["predictions"]
    assert _cabi.CALLS["track_update"] == before + 2
    want, ref = _reference_ids(preds)
    assert [p["track_ids"] for p in preds] == want
    assert ref.log["A"] > 10 and ref.log["started"] > 3
