"""CPU: tracking in the Inferencer -- how `tracker=` and `streams=` are read, the C entry points' argument contract, the
state layout, known answers of `track_ref` worked by hand, and the four two-state filters against a full 8x8 Kalman
filter in float64.  The kernel itself is compared with `track_ref` bit for bit in test_track_gpu.py."""
import ctypes
import glob
import os

import numpy as np
import pytest

import track_cases
from conftest import ROOT
from track_ref import F, TrackRef, iou

E_BADARG, E_TOO_LARGE = -1, -3
SWIN = glob.glob(os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py"))[0]


def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    return Inferencer(None, SWIN, dataset_meta=None, **kw)


# ---- 1. settings ------------------------------------------------------------------------------------------------------
def test_tracker_settings_defaults():
    from codetr import hip_ops
    from codetr.inferencer import tracker_settings

    assert tracker_settings(None) is None
    want = dict(obj_score_thrs=dict(high=0.6, low=0.1), init_track_thr=0.7, weight_iou_with_det_scores=True,
                match_iou_thrs=dict(high=0.1, low=0.5, tentative=0.3), num_frames_retain=30, num_tentatives=3,
                max_tracks=256)
    assert tracker_settings({}) == want == hip_ops.TRACKER
    assert hip_ops.TRACK_MAX_TRACKS == 512
    got = tracker_settings(dict(obj_score_thrs=dict(low=0.2), max_tracks=512, weight_iou_with_det_scores=0))
    assert got["obj_score_thrs"] == dict(high=0.6, low=0.2) and got["max_tracks"] == 512
    assert got["weight_iou_with_det_scores"] is False
    assert hip_ops.TRACKER["obj_score_thrs"]["low"] == 0.1   # the defaults are not written through
    assert _inferencer().tracker is None
    assert _inferencer(tracker=dict(num_tentatives=2)).tracker["num_tentatives"] == 2


@pytest.mark.parametrize("bad", [
    dict(unknown=1), dict(obj_score_thrs=dict(mid=0.5)), dict(match_iou_thrs=0.5), dict(obj_score_thrs=dict(high=float("nan"))),
    dict(init_track_thr=float("inf")), dict(init_track_thr="0.7"), dict(obj_score_thrs=dict(high=0.1, low=0.6)),
    dict(num_frames_retain=0), dict(num_tentatives=0), dict(num_tentatives=2.5), dict(max_tracks=0), dict(max_tracks=513),
    dict(max_tracks=True), "bytetrack", 3])
def test_tracker_settings_errors(bad):
    from codetr.inferencer import tracker_settings

    with pytest.raises(ValueError):
        tracker_settings(bad)
    with pytest.raises(ValueError):
        _inferencer(tracker=bad)


def test_tracker_from_config():
    from codetr.inferencer import tracker_settings

    with pytest.raises(ValueError, match="no tracker entry"):
        _inferencer(tracker="config")        # the shipped detection configs carry none
    cfg = dict(tracker=dict(type="ByteTracker", num_frames_retain=10, obj_score_thrs=dict(high=0.5, low=0.2)))
    got = tracker_settings("config", cfg)
    assert got["num_frames_retain"] == 10 and got["obj_score_thrs"] == dict(high=0.5, low=0.2)
    assert got["max_tracks"] == 256


def test_streams_validation():
    from codetr import hip_ops

    assert hip_ops.track_streams(None, 3) == [0, 0, 0]
    assert hip_ops.track_streams(5, 2) == [5, 5]
    assert hip_ops.track_streams([2, 0, 2], 3) == [2, 0, 2]
    assert hip_ops.track_streams(np.array([1, 7]), 2) == [1, 7]
    for bad in (-1, 1.0, "0", True, [0, 1], [0, -1, 2], [0, 1.5, 2], [0, None, 1], (0, 1, 2, 3)):
        with pytest.raises(ValueError):
            hip_ops.track_streams(bad, 3)
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    with pytest.raises(ValueError):          # validated before anything touches a device
        _inferencer(tracker={})(frames, streams=[0, -1])
    with pytest.raises(ValueError):
        _inferencer(tracker={})(frames, streams=[0])
    with pytest.raises(ValueError, match="without a tracker"):
        _inferencer()(frames, streams=0)
    inf = _inferencer(tracker={})
    inf.reset_tracks()                       # nothing to forget yet: no error
    inf.reset_tracks(4)
    with pytest.raises(ValueError):
        inf.reset_tracks(-2)


# ---- 2. the C entry points ---------------------------------------------------------------------------------------------
@pytest.fixture
def lib():
    from codetr import _cabi

    _cabi.RECORDER = []
    try:
        yield _cabi.load()
        assert _cabi.RECORDER == []   # no rejected call reached a launch
    finally:
        _cabi.RECORDER = None


def test_abi_number_constants_and_state_bytes(lib):
    from codetr import _cabi, hip_ops

    assert _cabi.ABI_VERSION == 54 and lib.codetr_hip_abi_version() == 54
    assert "track_update" in _cabi.CALLS
    header = open(os.path.join(ROOT, "include", "codetr_hip.h")).read()
    assert "#define CODETR_TRACK_MAX_TRACKS 512" in header
    assert "parity with mmdet is unpinned" in header
    # the stated layout: 4 int32, then per slot an int64, four int32, 8 + 12 floats
    for T in (1, 2, 7, 256, 512):
        assert lib.codetr_track_state_bytes(T) == 16 + T * (8 + 4 * 4 + 8 * 4 + 12 * 4) == _cabi.track_state_bytes(T)
    for T in (0, -1, 513, 2 ** 40):
        assert lib.codetr_track_state_bytes(T) == E_BADARG
    assert hip_ops.new_track_state(3, 7, "cpu").shape == (3, 16 + 104 * 7)
    host = hip_ops.track_state_to_host(hip_ops.new_track_state(3, 7, "cpu"))
    assert host.f.tolist() == [0, 0, 0] and host.next_id.tolist() == [1, 1, 1] and host.refused.tolist() == [0, 0, 0]
    assert host.id.shape == (3, 7) and host.label.dtype == np.int64 and host.mean.shape == (3, 7, 4, 2)
    assert host.cov.shape == (3, 7, 4, 3) and not host.cov.any()


def test_state_decoding_follows_the_stated_layout():
    """a state written by hand, field by field at the header's offsets, comes back through track_state_to_host"""
    import torch
    from codetr import hip_ops

    T = 3
    raw = np.zeros(16 + 104 * T, np.uint8)
    raw[:16].view(np.int32)[:] = (5, 9, 2, 0)
    raw[16:16 + 8 * T].view(np.int64)[:] = (11, 2 ** 40, 13)
    ints = raw[16 + 8 * T:16 + 24 * T].view(np.int32).reshape(4, T)
    ints[0], ints[1], ints[2], ints[3] = (1, 0, 3), (4, 5, 6), (0, 0, 1), (2, 3, 4)
    raw[16 + 24 * T:16 + 56 * T].view(np.float32)[:] = np.arange(8 * T)           # mean[8][T]
    raw[16 + 56 * T:].view(np.float32)[:] = 100 + np.arange(12 * T)               # cov[12][T]
    host = hip_ops.track_state_to_host(torch.from_numpy(raw)[None])
    assert (host.f[0], host.next_id[0], host.refused[0]) == (5, 10, 2)
    assert host.label[0].tolist() == [11, 2 ** 40, 13] and host.id[0].tolist() == [1, 0, 3]
    assert host.hits[0].tolist() == [4, 5, 6] and host.tentative[0].tolist() == [0, 0, 1]
    assert host.last[0].tolist() == [2, 3, 4]
    assert host.mean[0, 1].tolist() == [[1, 4], [7, 10], [13, 16], [19, 22]]      # slot 1: row 2 c + i at column 1
    assert host.cov[0, 2, 3].tolist() == [100 + 9 * T + 2, 100 + 10 * T + 2, 100 + 11 * T + 2]


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_track_update_rejects_bad_arguments(lib, suffix):
    f = getattr(lib, "codetr_track_update_" + suffix)
    one = ctypes.c_void_p(16)   # device pointers: never dereferenced, validation fails first
    thr = (0.6, 0.1, 0.7, 0.1, 0.5, 0.3)

    def call(ptrs=None, N=2, Q=300, streams=(0, 1), S=2, T=256, settings=thr, retain=30, tentatives=3):
        b, s, l, c, st, out = ptrs or [one] * 6
        table = None if streams is None else (ctypes.c_int * len(streams))(*streams)
        values = None if settings is None else (ctypes.c_float * 6)(*settings)
        return f(None, b, s, l, c, N, Q, table, S, st, T, values, retain, tentatives, 1, out)

    for i in range(6):
        ptrs = [one] * 6
        ptrs[i] = None
        assert call(ptrs) == E_BADARG, i
    assert call(streams=None) == E_BADARG
    assert call(settings=None) == E_BADARG
    for name in ("N", "Q", "S", "T"):
        assert call(**{name: 0}) == E_BADARG, name
        assert call(**{name: -4}) == E_BADARG, name
    assert call(streams=(0, 2)) == E_BADARG
    assert call(streams=(-1, 0)) == E_BADARG
    assert call(streams=(0, 1), S=1) == E_BADARG
    for i in range(6):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(settings=thr[:i] + (bad,) + thr[i + 1:]) == E_BADARG, i
    assert call(retain=0) == E_BADARG
    assert call(tentatives=0) == E_BADARG
    assert call(retain=-5) == E_BADARG
    assert call(N=33, streams=(0,) * 33) == E_TOO_LARGE       # CODETR_PREPROCESS_BATCH_MAX
    assert call(Q=1025) == E_TOO_LARGE                        # CODETR_POSTPROCESS_MAX_Q
    assert call(T=513) == E_TOO_LARGE                         # CODETR_TRACK_MAX_TRACKS


# ---- 3. known answers of the reference ---------------------------------------------------------------------------------
def _frame(ref, *rows):
    """rows of (x1, y1, x2, y2, score, label) -> the ids"""
    a = np.array(rows, np.float64).reshape(-1, 6)
    return ref.update(a[:, :4].astype(np.float32), a[:, 4].astype(np.float32), a[:, 5].astype(np.int64)).tolist()


def test_one_box_at_a_constant_step():
    """The box (100, 100, 140, 180) -- cx 120, cy 140, a 0.5, h 80 -- moves by +4 in x per frame, score 0.9.
    wp * 80: wp = fl(0.05) = 0.05 + 7.5e-10, the product 4 + 6e-8 rounds to 4; wv * 80 = 0.5 - 1.1e-8 rounds to 0.5.
    Frame 0 starts track 1, confirmed: cx has p = 120, v = 0, A = (2 * 4)^2 = 64, B = 0, C = (10 * 0.5)^2 = 25.
    Frame 1 predicts with h = 80: p = 120, A = ((64 + 0) + 25) + 4^2 = 105, B = 0 + 25 = 25, C = 25 + 0.5^2 = 25.25; the
    overlap with (104, 100, 144, 180) is 36 * 80 / (3200 + 3200 - 2880) = 2880 / 3520, times 0.9 well above 0.1: matched.
    Update with z = 124, r = 4^2: S = 121, k0 = fl(105 / 121), k1 = fl(25 / 121), y = 4:
    p = 120 + fl(k0 * 4), v = fl(k1 * 4), A = 105 - fl(k0 * 105), B = 25 - fl(k0 * 25), C = 25.25 - fl(k1 * 25)."""
    ref = TrackRef()
    assert _frame(ref, (100, 100, 140, 180, 0.9, 3)) == [1]
    s = ref.state()
    assert (s.f, s.next_id, s.refused) == (1, 2, 0)
    assert (s.id[0], s.label[0], s.hits[0], s.tentative[0], s.last[0]) == (1, 3, 1, 0, 0)
    assert s.mean[0, 0].tolist() == [120.0, 0.0] and s.cov[0, 0].tolist() == [64.0, 0.0, 25.0]
    assert s.mean[0].tolist() == [[120.0, 0.0], [140.0, 0.0], [0.5, 0.0], [80.0, 0.0]]
    assert s.cov[0, 2].tolist() == [float(F(1e-2) * F(1e-2)), 0.0, float(F(1e-5) * F(1e-5))]
    assert s.cov[0, 3].tolist() == [64.0, 0.0, 25.0]
    assert float(iou((100, 100, 140, 180), tuple(F(v) for v in (104, 100, 144, 180)))) == float(F(2880) / F(3520))

    assert _frame(ref, (104, 100, 144, 180, 0.9, 3)) == [1]
    s = ref.state()
    k0, k1 = F(105) / F(121), F(25) / F(121)
    want_mean = [F(120) + k0 * F(4), k1 * F(4)]
    want_cov = [F(105) - k0 * F(105), F(25) - k0 * F(25), F(25.25) - k1 * F(25)]
    assert s.mean[0, 0].tolist() == [float(v) for v in want_mean]
    assert s.cov[0, 0].tolist() == [float(v) for v in want_cov]
    assert abs(s.mean[0, 0, 0] - 123.47107) < 1e-4 and abs(s.mean[0, 0, 1] - 0.826446) < 1e-5
    assert abs(s.cov[0, 0, 0] - 13.884298) < 1e-4 and abs(s.cov[0, 0, 2] - 20.084711) < 1e-4
    assert (s.hits[0], s.last[0], s.f) == (2, 1, 2)

    assert _frame(ref, (108, 100, 148, 180, 0.9, 3)) == [1]
    assert ref.state().hits[0] == 3 and ref.state().next_id == 2


def test_hidden_object_returns_within_the_retention():
    """num_frames_retain = 4.  Seen on frame 0; hidden on frames 1..3 (3 = retain - 1 frames): on frame 4 f - last = 4
    would retire it, but it is matched first (step 3 comes before step 7) and keeps id 1.  Hidden on frames 1..4: the
    slot is freed on frame 4 (f - last = 4 >= 4), so on frame 5 the box starts track 2, tentative as any start after
    frame 0."""
    box = (100, 100, 140, 180, 0.9, 0)
    for hidden, want in ((3, 1), (4, -2)):
        ref = TrackRef(dict(num_frames_retain=4))
        assert _frame(ref, box) == [1]
        for _ in range(hidden):
            assert _frame(ref) == []
        assert _frame(ref, box) == [want], hidden
        assert ref.log["retired"] == (1 if hidden == 4 else 0)


def test_unmatched_tentative_track_is_gone_and_its_id_is_not_reused():
    """Frame 0: A starts track 1.  Frame 1: B appears -> track 2, tentative (-2).  Frame 2: B is absent -> track 2 is
    freed.  Frame 3: B again -> a new tentative track with id 3, not 2, in the slot track 2 left (slot 1)."""
    ref = TrackRef()
    A, B = (100, 100, 140, 180, 0.9, 0), (300, 300, 340, 380, 0.9, 0)
    assert _frame(ref, A) == [1]
    assert _frame(ref, A, B) == [1, -2]
    assert _frame(ref, A) == [1]
    assert ref.state().id.tolist()[:3] == [1, 0, 0] and ref.log["tentative_removed"] == 1
    assert _frame(ref, A, B) == [1, -3]
    assert ref.state().id.tolist()[:3] == [1, 3, 0]
    assert _frame(ref, A, B) == [1, -3]
    assert _frame(ref, A, B) == [1, 3]           # hits = 3 = num_tentatives: confirmed
    assert ref.log["promoted"] == 1


def test_low_score_candidate():
    """A candidate of score 0.3 (0.1 < 0.3 <= 0.6) is `low`: it keeps the confirmed track of frame 0 alive through match
    C (IoU 1 >= 0.5), it starts nothing where no track is, and it is not given to a track that missed the previous
    frame: after an empty frame 2 the same low box on frame 3 gets id 0 -- while a high one on frame 4 still finds the
    lost track through match A."""
    ref = TrackRef()
    hi, lo, other = (100, 100, 140, 180, 0.9, 0), (100, 100, 140, 180, 0.3, 0), (300, 300, 340, 380, 0.3, 0)
    assert _frame(ref, hi) == [1]
    assert _frame(ref, lo, other) == [1, 0]
    assert ref.log["C"] == 1 and ref.state().hits[0] == 2 and ref.state().next_id == 2
    assert _frame(ref) == []
    assert _frame(ref, lo) == [0]
    assert ref.log["C"] == 1
    assert _frame(ref, hi) == [1]
    assert ref.log["A"] == 1


def test_overlapping_boxes_of_two_labels_keep_their_ids():
    """two boxes 4 px apart (IoU 0.82) with labels 0 and 1 that swap places from frame to frame: each track's nearer
    candidate has the other label, and labels are compared, so the ids follow the labels"""
    ref = TrackRef()
    p, q = (100, 100, 140, 180), (104, 100, 144, 180)
    assert _frame(ref, p + (0.9, 0), q + (0.8, 1)) == [1, 2]
    assert _frame(ref, q + (0.9, 0), p + (0.8, 1)) == [1, 2]
    assert _frame(ref, p + (0.8, 1), q + (0.9, 0)) == [2, 1]
    assert ref.state().label.tolist()[:2] == [0, 1] and ref.state().next_id == 3


def test_a_candidate_taken_in_match_a_is_not_offered_in_match_b():
    """Frame 0: P starts track 1.  Frame 1: P and P' (P shifted by 8 px, IoU 32 * 80 / (6400 - 2560) = 0.67): track 1
    takes the exact P (value 0.9 against 0.6), P' starts the tentative track 2.  Frame 2 shows P alone: track 1 takes it
    in match A, and match B, whose tentative track 2 overlaps P by far more than 0.3, finds no free candidate -- track 2
    is freed, and the row carries id 1, not -2."""
    ref = TrackRef()
    P, P2 = (100, 100, 140, 180, 0.9, 0), (108, 100, 148, 180, 0.9, 0)
    assert _frame(ref, P) == [1]
    assert _frame(ref, P, P2) == [1, -2]
    assert _frame(ref, P) == [1]
    assert ref.log["B"] == 0 and ref.log["tentative_removed"] == 1 and ref.state().id.tolist()[:2] == [1, 0]


def test_the_third_start_is_refused_with_two_slots():
    ref = TrackRef(dict(max_tracks=2))
    rows = [(100 * k, 100, 100 * k + 40, 180, 0.9, 0) for k in range(1, 4)]
    assert _frame(ref, *rows) == [1, 2, 0]
    s = ref.state()
    assert (s.refused, s.next_id) == (1, 3) and s.id.tolist() == [1, 2]
    assert _frame(ref, *rows) == [1, 2, 0]
    assert ref.state().refused == 2 and ref.state().next_id == 3


def test_the_scripted_sequences_take_every_branch():
    """what test_track_gpu.py relies on, checked where it is cheap"""
    import torch

    b, s, l, c = track_cases.cached_sequence("reference")
    assert b.shape == (12, 48, 4) and c.min() == 0 and len(set(c.tolist())) > 3 and set(l.flatten().tolist()) == {0, 1, 2}
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        _, _, log = track_cases.run_reference(torch.tensor(b).to(dtype), torch.tensor(s).to(dtype), l, c,
                                              track_cases.SETTINGS)
        track_cases.assert_exercises_every_branch(log)
    b, s, l, c = track_cases.cached_sequence("dense")
    above = int((s[0] > 0.7).sum())
    assert above > 512
    _, state, log = track_cases.run_reference(b.astype(np.float32), s.astype(np.float32), l, c, dict(max_tracks=512))
    assert log["refused"] >= above - 512 > 0 and (state.id != 0).all()


# ---- 4. four two-state filters = one 8x8 filter ------------------------------------------------------------------------
class Kalman8:
    """mmdet's KalmanFilter (the SORT filter: state (cx, cy, a, h) and its velocities) with full matrices in float64"""
    WP, WV = 1.0 / 20, 1.0 / 160

    def __init__(self, z):
        self.F = np.eye(8)
        self.F[:4, 4:] = np.eye(4)
        self.H = np.eye(4, 8)
        self.mean = np.r_[z, np.zeros(4)]
        h = z[3]
        std = [2 * self.WP * h, 2 * self.WP * h, 1e-2, 2 * self.WP * h, 10 * self.WV * h, 10 * self.WV * h, 1e-5, 10 * self.WV * h]
        self.cov = np.diag(np.square(std))

    def predict(self):
        h = self.mean[3]
        std = [self.WP * h, self.WP * h, 1e-2, self.WP * h, self.WV * h, self.WV * h, 1e-5, self.WV * h]
        self.mean = self.F @ self.mean
        self.cov = self.F @ self.cov @ self.F.T + np.diag(np.square(std))

    def update(self, z):
        h = self.mean[3]
        R = np.diag(np.square([self.WP * h, self.WP * h, 1e-1, self.WP * h]))
        S = self.H @ self.cov @ self.H.T + R
        K = self.cov @ self.H.T @ np.linalg.inv(S)
        self.mean = self.mean + K @ (z - self.H @ self.mean)
        self.cov = self.cov - K @ S @ K.T


def test_four_two_state_filters_against_the_full_filter():
    """One object over 50 frames: centre (200 + 3 f, 150 + 2 f), size about 60 x 120, uniform noise of +-2 px on every
    edge.  The fp32 filters of track_ref against the float64 8x8 filter fed the same float32 measurements.
    Measured on an x86-64 CPU (numpy 2): the largest deviation of a mean component over the 50 frames is 3.02e-5 (on cx at
    frame 36, where cx is 308: one ulp of fp32 there), so the bound is 4 * 3.02e-5 = 1.21e-4; the margin covers
    summation-order differences between numpy builds.  A wrong noise term misses by orders of magnitude more: with the
    velocity weight 1/160 of the full filter replaced by 1/16 the deviation is 1.9."""
    rng = np.random.default_rng(3)
    ref, full, worst = TrackRef(), None, 0.0
    for f in range(50):
        cx, cy = 200 + 3 * f, 150 + 2 * f
        box = np.array([cx - 30, cy - 60, cx + 30, cy + 60]) + rng.uniform(-2, 2, 4)
        box = box.astype(np.float32)
        assert ref.update(box[None], np.array([0.9], np.float32), np.array([0])).tolist() == [1]
        x1, y1, x2, y2 = box.astype(np.float64)
        z = np.array([(x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1) / (y2 - y1), y2 - y1])
        if full is None:
            full = Kalman8(z)
        else:
            full.predict()
            full.update(z)
        got = ref.state().mean[0].astype(np.float64)          # [4, 2]: p then v
        worst = max(worst, np.abs(got[:, 0] - full.mean[:4]).max(), np.abs(got[:, 1] - full.mean[4:]).max())
    print(f"largest deviation of the mean: {worst:.3e}")
    assert worst <= 4 * 3.02e-5
    # the covariances: the off-diagonal blocks between coordinates stay exactly zero in the full filter
    blocks = full.cov.reshape(2, 4, 2, 4)
    for a in range(4):
        for b in range(4):
            if a != b:
                assert not blocks[:, a, :, b].any()
