"""GPU: the assignment kernel (codetr_assign_i32, hip_ops.linear_assignment) and the tracker's optimal association
(codetr_track_update2_*, Inferencer(track_association="optimal")).  Matches equal the numpy restatements element for
element (tests/assign_ref.py, tests/track_assign_ref.py), totals equal scipy's optimum, the greedy mode of the new
entry equals the old entry byte for byte.  Output buffers are sentinel-filled between guard rows."""
import numpy as np
import pytest
import torch

import assign_ref
import track_assign_cases as cases
import track_cases
from test_assign_cpu import random_gains
from test_inferencer_batch_gpu import DEV, SWIN, _same
from test_track_gpu import (DTYPES, SENTINEL_BYTE, SENTINEL_ID, Device, _assert_rows_beyond_count_are_zero,
                            _assert_state, _frames, _rounded, _stub, _thresholds)
from track_assign_ref import TrackAssignRef
from track_ref import TrackRef

pytestmark = pytest.mark.gpu


# ---- 1. the solver -------------------------------------------------------------------------------------------------------
def _solve_on_device(G):
    """G [B, n, m] int64 on the host -> (match [B, n], total [B]) through codetr_assign_i32, guard rows checked"""
    from codetr import _assign, _cabi

    B, n, m = G.shape
    gain = torch.as_tensor(G.astype(np.int32)).to(DEV)
    match = torch.full((B + 2, n), SENTINEL_ID, dtype=torch.int32, device=DEV)
    total = torch.full((B + 2,), -7, dtype=torch.int64, device=DEV)
    before = _cabi.CALLS["assign"]
    _assign.assign(gain, match[1:-1], total[1:-1])
    assert _cabi.CALLS["assign"] == before + 1
    torch.cuda.synchronize()
    mh, th = match.cpu().numpy(), total.cpu().numpy()
    assert (mh[0] == SENTINEL_ID).all() and (mh[-1] == SENTINEL_ID).all() and th[0] == th[-1] == -7
    return mh[1:-1], th[1:-1]


def _check(G):
    G = np.asarray(G, np.int64)
    G = G[None] if G.ndim == 2 else G
    match, total = _solve_on_device(G)
    for b in range(G.shape[0]):
        want, want_total, _ = assign_ref.solve(G[b])
        assert np.array_equal(match[b], want), b                      # the stated matching, not just an optimum
        assert total[b] == want_total == assign_ref.optimum(G[b]), b  # and scipy's optimum
        assert assign_ref.check_matching(G[b], match[b]) == total[b]


@pytest.mark.parametrize("n,m", [(1, 1), (3, 5), (5, 3), (64, 64), (65, 130), (257, 300)])
def test_random_dense(n, m):
    """(257, 300) crosses the 256-thread ownership of columns; (5, 3) needs virtual columns"""
    rng = np.random.default_rng(n * 1000 + m)
    _check(random_gains(rng, n, m))
    _check(random_gains(rng, n, m, hi=3))          # ties everywhere


def test_largest_sparse():
    _check(random_gains(np.random.default_rng(1), 512, 1024, density=0.02))


def test_more_rows_than_columns_at_the_limits():
    _check(random_gains(np.random.default_rng(2), 512, 200, density=0.05))


def test_zero_matrices_and_three_problems_in_one_launch():
    rng = np.random.default_rng(3)
    _check(np.zeros((7, 9), np.int64))
    G = random_gains(rng, 12, 9)
    G[[0, 5, 11]] = 0
    _check(G)
    G = np.stack([random_gains(rng, 40, 70), random_gains(rng, 40, 70, density=0.05), np.full((40, 70), 9)])
    _check(G)
    _check(np.array([[-5, 3], [2 ** 30, 2 ** 30]]))    # clamped as they are read


@pytest.mark.parametrize("kind", ["equal", "outer"])
def test_structured_128(kind):
    """8,256 rounds each: row i walks the i columns taken before it"""
    k = np.arange(1, 129)
    G = np.full((128, 128), 1000) if kind == "equal" else np.outer(k, k)
    assert assign_ref.solve(G)[2] == 8256
    _check(G)


def test_all_equal_512():
    """131,328 rounds: row i walks the i columns taken before it.  Measured on an MI355X: 0.81 s for this whole test
    (upload, launch, download, the numpy restatement and scipy on the host); at the measured 1.6 us per round the launch
    itself is about 0.21 s.  Under two seconds, so the 512 x 512 form stays (profiles/r19_track_assign.txt)."""
    G = np.full((512, 512), 12345)
    _check(G)


def test_linear_assignment_operator():
    from codetr import hip_ops

    rng = np.random.default_rng(4)
    G = random_gains(rng, 100, 900, density=0.1)                       # a DETR matcher's shape
    match, total = hip_ops.linear_assignment(torch.as_tensor(G.astype(np.int32)).to(DEV))
    want, want_total, _ = assign_ref.solve(G)
    assert match.shape == (100,) and match.dtype == torch.int32 and total.shape == () and total.dtype == torch.int64
    assert np.array_equal(match.cpu().numpy(), want) and int(total) == want_total == assign_ref.optimum(G)
    Gs = np.stack([random_gains(rng, 9, 6), random_gains(rng, 9, 6)])
    match, total = hip_ops.linear_assignment(torch.as_tensor(Gs.astype(np.int32)).to(DEV).transpose(1, 2).contiguous().transpose(1, 2))
    for b in range(2):
        assert np.array_equal(match[b].cpu().numpy(), assign_ref.solve(Gs[b])[0]) and int(total[b]) == assign_ref.optimum(Gs[b])
    empty = hip_ops.linear_assignment(torch.zeros((3, 0), dtype=torch.int32, device=DEV))
    assert empty[0].tolist() == [-1, -1, -1] and int(empty[1]) == 0


# ---- 2. the tracker ------------------------------------------------------------------------------------------------------
class Device2(Device):
    """test_track_gpu's Device, launching codetr_track_update2_* with an association"""

    def __init__(self, S, settings, association="optimal"):
        super().__init__(S, settings)
        self.association = association

    def launch(self, boxes, scores, labels, count, streams):
        from codetr import _assign, _cabi

        N, Q = scores.shape
        ids = torch.full((N + 2, Q), SENTINEL_ID, dtype=torch.int32, device=DEV)
        before = _cabi.CALLS["track_update2"], _cabi.CALLS["track_update"]
        _assign.track_update2(boxes.to(DEV).contiguous(), scores.to(DEV).contiguous(),
                              torch.as_tensor(labels).to(DEV).contiguous(), torch.as_tensor(count).to(DEV).contiguous(),
                              streams, self.state, self.T, _thresholds(self.cfg), self.cfg["num_frames_retain"],
                              self.cfg["num_tentatives"], self.cfg["weight_iou_with_det_scores"], ids[1:-1],
                              _assign.ASSOCIATIONS[self.association])
        assert (_cabi.CALLS["track_update2"], _cabi.CALLS["track_update"]) == (before[0] + 1, before[1])
        torch.cuda.synchronize()
        host = ids.cpu().numpy()
        assert (host[0] == SENTINEL_ID).all() and (host[-1] == SENTINEL_ID).all()
        assert (host[1:-1] != SENTINEL_ID).all()
        return host[1:-1]


def _tensors(seq, dtype):
    b, s, l, c = seq
    return torch.tensor(b).to(dtype), torch.tensor(s).to(dtype), l, c


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_sequence_optimal(dtype):
    seq = _rounded("reference", dtype)
    want_ids, want_state, log = cases.run(TrackAssignRef, *seq, track_cases.SETTINGS)
    assert log["A"] > 50 and log["B"] > 0 and log["C"] > 0 and log["refused"] > 0 and log["problems"] > 12
    dev = Device2(1, track_cases.SETTINGS)
    ids = dev.run(seq, [12])
    assert np.array_equal(ids, want_ids)
    _assert_rows_beyond_count_are_zero(ids, seq[3])
    _assert_state(dev.decoded(), 0, want_state)


@pytest.mark.parametrize("dtype", DTYPES)
def test_greedy_through_the_new_entry_equals_the_old_entry(dtype):
    seq = _rounded("reference", dtype)
    old, new = Device(1, track_cases.SETTINGS), Device2(1, track_cases.SETTINGS, "greedy")
    assert np.array_equal(old.run(seq, [5, 7]), new.run(seq, [5, 7]))
    old.decoded(), new.decoded()
    assert np.array_equal(old.state.cpu().numpy(), new.state.cpu().numpy())     # the state, byte for byte


def test_crossing_case():
    seq = _tensors(cases.crossing_case(), torch.float32)
    want_o = cases.run(TrackAssignRef, *seq, None)
    want_g = cases.run(TrackRef, *seq, None)
    assert want_o[0][1].tolist() == [2, 1] and want_g[0][1].tolist() == [1, -3]
    for association, want in (("optimal", want_o), ("greedy", want_g)):
        dev = Device2(1, None, association)
        assert np.array_equal(dev.run(seq, [3]), want[0]), association
        _assert_state(dev.decoded(), 0, want[1])
    # a stream may switch association between calls: frame 0 greedy, then optimal -- frame 0 has nothing to associate
    dev = Device2(1, None, "greedy")
    first = dev.launch(seq[0][:1], seq[1][:1], seq[2][:1], seq[3][:1], [0])
    dev.association = "optimal"
    rest = dev.launch(seq[0][1:], seq[1][1:], seq[2][1:], seq[3][1:], [0, 0])
    assert np.array_equal(np.concatenate((first, rest)), want_o[0])
    # and through hip_ops.track_update
    from codetr import hip_ops

    state = hip_ops.new_track_state(1, 256, DEV)
    dets = hip_ops.Detections(seq[0].to(DEV), seq[1].to(DEV), torch.as_tensor(seq[2]).to(DEV), torch.as_tensor(seq[3]).to(DEV), None)
    assert np.array_equal(hip_ops.track_update(dets, state, association="optimal").cpu().numpy(), want_o[0])
    state.zero_()
    assert np.array_equal(hip_ops.track_update(dets, state).cpu().numpy(), want_g[0])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_crowd_where_greedy_and_optimal_disagree(dtype):
    seq = _tensors(cases.cached_crowd(), dtype)
    settings = dict(max_tracks=64)
    want_ids, want_state, log = cases.run(TrackAssignRef, *seq, settings)
    greedy_ids, _, _ = cases.run(TrackRef, *seq, settings)
    differing = [f for f in range(len(seq[3])) if not np.array_equal(greedy_ids[f], want_ids[f])]
    assert len(differing) >= 2 and log["rounds"] > 2 * log["A"] > 100      # the case has not degenerated into greedy
    dev = Device2(1, settings)
    assert np.array_equal(dev.run(seq, [8]), want_ids)
    _assert_state(dev.decoded(), 0, want_state)
    dev = Device2(1, settings, "greedy")
    assert np.array_equal(dev.run(seq, [8]), greedy_ids)


def test_chunking_does_not_matter_optimal():
    seq = _tensors(cases.cached_crowd(), torch.float16)
    settings = dict(max_tracks=64)
    want_ids, want_state, _ = cases.run(TrackAssignRef, *seq, settings)
    raws = []
    for chunks in ([8], [1] * 8, [3, 5]):
        dev = Device2(1, settings)
        assert np.array_equal(dev.run(seq, chunks), want_ids)
        _assert_state(dev.decoded(), 0, want_state)
        raws.append(dev.state.cpu().numpy())
    assert np.array_equal(raws[0], raws[1]) and np.array_equal(raws[0], raws[2])


def test_two_streams_in_one_launch_optimal():
    dtype = torch.float16
    a, b = _rounded("reference", dtype), _rounded("second", dtype)
    want = [cases.run(TrackAssignRef, *s, track_cases.SETTINGS) for s in (a, b)]
    boxes, scores = torch.stack((a[0], b[0]), 1).flatten(0, 1), torch.stack((a[1], b[1]), 1).flatten(0, 1)
    labels, count = np.stack((a[2], b[2]), 1).reshape(24, -1), np.stack((a[3], b[3]), 1).reshape(24)
    dev = Device2(3, track_cases.SETTINGS)
    dev.state[1].fill_(SENTINEL_BYTE)                       # stream 1 has no row in this launch
    ids = dev.launch(boxes, scores, labels, count, [2, 0] * 12)
    assert np.array_equal(ids[0::2], want[0][0]) and np.array_equal(ids[1::2], want[1][0])
    got = dev.decoded()
    _assert_state(got, 2, want[0][1])
    _assert_state(got, 0, want[1][1])
    assert (dev.state[1].cpu().numpy() == SENTINEL_BYTE).all()


def test_limits_large_optimal():
    """T = 512 with Q = 1024: two tracks and four columns per thread, 114 KB of LDS"""
    b, s, l, c = track_cases.cached_sequence("dense")
    seq = (torch.tensor(b).float(), torch.tensor(s).float(), l, c)
    settings = dict(max_tracks=512)
    want_ids, want_state, log = cases.run(TrackAssignRef, *seq, settings)
    assert log["refused"] > 0 and log["A"] > 256 and log["C"] > 0
    dev = Device2(1, settings)
    assert np.array_equal(dev.run(seq, [3]), want_ids)
    _assert_state(dev.decoded(), 0, want_state)


@pytest.mark.parametrize("Q", [640, 656, 688])
def test_around_the_64_kb_lds_threshold_optimal(Q):
    """256 slots: the kernel's LDS (the tracker's + 8 T + 12 Q + 96) is 63 856 bytes at Q = 640, 64 576 at 656 -- under
    64 KB on its own, over it with what the compiler adds -- and 66 016 at 688: each side of the opt-in must launch"""
    b, s, l, c = track_cases.dense_sequence(frames=2, Q=Q)
    seq = (torch.tensor(b).float(), torch.tensor(s).float(), l, c)
    want_ids, want_state, log = cases.run(TrackAssignRef, *seq, dict(max_tracks=256))
    assert log["refused"] > 0 and log["A"] > 128
    dev = Device2(1, dict(max_tracks=256))
    assert np.array_equal(dev.run(seq, [2]), want_ids)
    _assert_state(dev.decoded(), 0, want_state)


# ---- 3. the Inferencer ---------------------------------------------------------------------------------------------------
def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    inf = Inferencer(None, SWIN, dataset_meta=None, **kw)
    inf.model = _stub(inf)
    return inf


def _reference_ids(preds, cls):
    ref, out = cls(None), []
    for p in preds:
        n = len(p["labels"])
        ids = ref.update(np.asarray(p["bboxes"], np.float32).reshape(n, 4), np.asarray(p["scores"], np.float32),
                         np.asarray(p["labels"], np.int64))
        out.append(ids.tolist())
    return out, ref


@pytest.mark.parametrize("kw", [dict(), dict(slicing=dict(tile=(96, 96), overlap=0.25))], ids=["plain", "sliced"])
def test_inferencer_optimal(kw):
    from codetr import _cabi

    inf = _inferencer(tracker={}, track_association="optimal", **kw)
    before = _cabi.CALLS["track_update2"], _cabi.CALLS["track_update"]
    preds = inf(_frames(range(6)), device=DEV, dtype=torch.float16, batch_size=3)["predictions"]
    assert (_cabi.CALLS["track_update2"], _cabi.CALLS["track_update"]) == (before[0] + 2, before[1])   # one launch per chunk
    want, ref = _reference_ids(preds, TrackAssignRef)
    assert [p["track_ids"] for p in preds] == want
    assert ref.log["A"] > 10 and ref.log["started"] > 3 and ref.log["problems"] >= 5
    # the default stays greedy: the old entry, TrackRef's ids, the same detections
    greedy = _inferencer(tracker={}, **kw)(_frames(range(6)), device=DEV, dtype=torch.float16, batch_size=3)["predictions"]
    assert _cabi.CALLS["track_update2"] == before[0] + 2 and _cabi.CALLS["track_update"] == before[1] + 2
    assert [p["track_ids"] for p in greedy] == _reference_ids(greedy, TrackRef)[0]
    _same(greedy, preds)
