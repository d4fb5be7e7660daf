"""The Inferencer's tracking operators (hip_ops re-exports them): the tracker's update and its state, the camera-motion
estimate, the appearance descriptors, and the assignment solver.  GPU-only, as hip_ops.
"""
import collections
import math

import numpy as np
import torch

from . import _appearance, _assign, _cabi, _motion
from . import _operands as _check
from ._operands import _gpu

# the public names (hip_ops re-exports exactly these)
__all__ = [
    "TRACK_MAX_TRACKS", "TRACKER", "TrackState", "track_settings", "new_track_state", "track_state_to_host",
    "TRACK_ASSOCIATIONS", "APPEARANCE", "APPEARANCE_BINS", "appearance_settings", "appearance_descriptors",
    "new_appearance_state", "appearance_state_to_host", "track_update", "estimate_motion", "MOTION",
    "MOTION_MODELS", "MotionState", "motion_settings", "new_motion_state", "motion_state_to_host",
    "ASSIGN_MAX_GAIN", "ASSIGN_MAX_COLS", "ASSIGN_MAX_ROWS", "linear_assignment", "track_streams",
]

TRACK_MAX_TRACKS = _cabi.TRACK_MAX_TRACKS
# this build's defaults: mmdet's ByteTracker config values as recalled (unpinned: mmdet is not installed here); max_tracks
# is this build's own
TRACKER = dict(obj_score_thrs=dict(high=0.6, low=0.1), init_track_thr=0.7, weight_iou_with_det_scores=True,
               match_iou_thrs=dict(high=0.1, low=0.5, tentative=0.3), num_frames_retain=30, num_tentatives=3,
               max_tracks=256)
TrackState = collections.namedtuple("TrackState", "f next_id refused id label hits tentative last mean cov")


def track_settings(settings=None):
    """the settings of track_update, validated and completed from TRACKER (a partial obj_score_thrs / match_iou_thrs
    dict keeps the other defaults) -> a new dict.  ValueError for an unknown key, a threshold that is not a finite
    number, obj_score_thrs.low > high, num_frames_retain or num_tentatives < 1 or not an integer, max_tracks outside
    1..TRACK_MAX_TRACKS."""
    def thresholds(key):
        def check(v):
            if not isinstance(v, dict) or set(v) - set(TRACKER[key]):
                raise ValueError(f"tracker {key}: a dict with keys of {sorted(TRACKER[key])}")
            return _check.validated(f"tracker {key}", TRACKER[key], v, dict.fromkeys(TRACKER[key], _check.number()), sep=".")
        return check

    count = _check.whole(1, 2 ** 31 - 1)
    out = _check.validated("tracker", TRACKER, settings, dict(
        obj_score_thrs=thresholds("obj_score_thrs"), match_iou_thrs=thresholds("match_iou_thrs"),
        init_track_thr=_check.number(), weight_iou_with_det_scores=bool, num_frames_retain=count, num_tentatives=count,
        max_tracks=_check.whole(1, TRACK_MAX_TRACKS)))
    if out["obj_score_thrs"]["low"] > out["obj_score_thrs"]["high"]:
        raise ValueError("tracker obj_score_thrs: low must not exceed high")
    return out


def new_track_state(S, max_tracks, device):
    """the states of S fresh streams of max_tracks slots each: zeros [S, 16 + 104 max_tracks] uint8 on `device`
    (include/codetr_hip.h states the layout; track_state_to_host decodes it)"""
    if int(S) < 1:
        raise ValueError(f"new_track_state: at least one stream, got {S}")
    if not 1 <= int(max_tracks) <= TRACK_MAX_TRACKS:
        raise ValueError(f"new_track_state: max_tracks in 1..{TRACK_MAX_TRACKS}, got {max_tracks}")
    return torch.zeros((int(S), _cabi.track_state_bytes(max_tracks)), dtype=torch.uint8, device=device)


def _track_slots(state):
    if not torch.is_tensor(state) or state.dtype != torch.uint8 or state.dim() != 2 or not state.is_contiguous() or \
            state.shape[0] < 1 or state.shape[1] < 120 or (state.shape[1] - 16) % 104:
        raise ValueError("track state: a contiguous [S, 16 + 104 max_tracks] uint8 tensor (new_track_state)")
    return (state.shape[1] - 16) // 104


def track_state_to_host(state):
    """the states of new_track_state / track_update decoded on the host (one device-to-host copy) -> TrackState of numpy
    arrays: f, next_id, refused [S]; id, hits, tentative, last (int32) and label (int64) [S, T]; mean [S, T, 4, 2] (p, v of
    cx, cy, a, h) and cov [S, T, 4, 3] (A, B, C) float32"""
    T = _track_slots(state)
    raw = state.cpu().numpy()
    S = raw.shape[0]
    hdr = raw[:, :16].copy().view(np.int32)
    o = 16
    label = raw[:, o:o + 8 * T].copy().view(np.int64)
    o += 8 * T
    ints = raw[:, o:o + 16 * T].copy().view(np.int32).reshape(S, 4, T)
    o += 16 * T
    mean = raw[:, o:o + 32 * T].copy().view(np.float32).reshape(S, 4, 2, T).transpose(0, 3, 1, 2).copy()
    o += 32 * T
    cov = raw[:, o:o + 48 * T].copy().view(np.float32).reshape(S, 4, 3, T).transpose(0, 3, 1, 2).copy()
    return TrackState(hdr[:, 0].copy(), hdr[:, 1] + 1, hdr[:, 2].copy(), ints[:, 0].copy(), label, ints[:, 1].copy(),
                      ints[:, 2].copy(), ints[:, 3].copy(), mean, cov)


TRACK_ASSOCIATIONS = tuple(_assign.ASSOCIATIONS)   # "greedy" (the default, codetr_hip.h's rule) and "optimal"

# the appearance cue (include/codetr_appearance.h states the rule, these settings' ranges and the cue's limits).  The two
# thresholds are BoT-SORT's appearance_thresh (0.25, as a distance) and proximity_thresh as recalled (unpinned: BoT-SORT
# is not installed here); reid_gate is this library's own
APPEARANCE = dict(appearance_thr=0.75, proximity_thr=0.5, reid_gate=1.5)
APPEARANCE_BINS = _appearance.BINS


def appearance_settings(d=None):
    """the settings of the appearance cue, validated and completed from APPEARANCE -> a new dict.  ValueError for an
    unknown key or a value that is not a finite number of its range: the thresholds in [0, 1], reid_gate >= 0."""
    return _check.validated("appearance", APPEARANCE, d, dict(
        appearance_thr=_check.number(0, 1.0), proximity_thr=_check.number(0, 1.0), reid_gate=_check.number(0, math.inf)))


_appearance_settings = appearance_settings   # (track_update has an argument of that name)


def appearance_descriptors(src_u8, rows, dets):
    """The colour descriptor of every detection in one launch per PREPROCESS_BATCH_MAX rows and without a synchronisation
    (csrc/appearance.hip; include/codetr_appearance.h states the rule: 16 x 32 samples over the inner three quarters of
    the box, two stripes of 64 two-bit RGB bins).
      src_u8  one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows    (offset, H, W) per image, one per row of the detections
      dets    Detections / SoftDetections over [N, Q] rows in source pixels (boxes and count are read)
    -> [N, Q, 128] int16 on the device (the header's uint16 bits: a value is at most 256); zeros for a row beyond count,
    with a non-finite coordinate or without area."""
    _gpu(src_u8, "appearance_descriptors")
    rows = _check.image_rows("appearance_descriptors", src_u8, rows, _cabi.FRAME_MAX_SIDE)
    boxes = dets.boxes
    if not torch.is_tensor(boxes) or boxes.dtype not in _check.FLOATS or \
            boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.device != src_u8.device:
        raise ValueError("appearance_descriptors: boxes [N, Q, 4] in f16, bf16 or f32 on the images' device")
    N, Q = boxes.shape[:2]
    if len(rows) != N or tuple(dets.count.shape) != (N,):
        raise ValueError(f"appearance_descriptors: one image row and one count per detection row ({N})")
    if Q > _cabi.POSTPROCESS_MAX_Q:
        raise ValueError(f"appearance_descriptors: at most {_cabi.POSTPROCESS_MAX_Q} detection rows per frame, got {Q}")
    desc = torch.empty((N, Q, _appearance.BINS), dtype=torch.int16, device=src_u8.device)
    if N == 0 or Q == 0:
        return desc
    boxes, count = boxes.contiguous(), dets.count.contiguous()
    with torch.cuda.device(src_u8.device):
        for i, j in _check.chunks(N):
            _appearance.describe(src_u8, rows[i:j], boxes[i:j], count[i:j], desc[i:j])
    return desc


def new_appearance_state(S, max_tracks, device):
    """the appearance states of S fresh streams of max_tracks slots each: zeros [S, max_tracks, 128] int16 on `device`
    (the header's uint16 in sixteenths; appearance_state_to_host decodes it)"""
    if int(S) < 1:
        raise ValueError(f"new_appearance_state: at least one stream, got {S}")
    if not 1 <= int(max_tracks) <= TRACK_MAX_TRACKS:
        raise ValueError(f"new_appearance_state: max_tracks in 1..{TRACK_MAX_TRACKS}, got {max_tracks}")
    return torch.zeros((int(S), int(max_tracks), _appearance.BINS), dtype=torch.int16, device=device)


def appearance_state_to_host(state):
    """the states of new_appearance_state / track_update on the host (one device-to-host copy) -> [S, T, 128] numpy
    uint16"""
    return state.cpu().numpy().view(np.uint16).copy()


def track_update(dets, state, streams=None, settings=None, association="greedy", motion=None, appearance=None,
                 appearance_state=None, appearance_settings=None):
    """Tracking-by-detection for the frames of a chunk in one launch per PREPROCESS_BATCH_MAX rows (track_kernel in
    csrc/track.hip, one kernel text instantiated per form of the update; the rule, modelled on mmdet's ByteTracker, is
    stated in include/codetr_hip.h): the three greedy associations, the Kalman filters, retirement and track starts of
    every stream on the device.
      dets      Detections / SoftDetections over [N, Q] rows, Q <= 1024: whatever the chunk's last launch produced
      state     new_track_state's tensor, updated in place; it stays on the device between calls
      streams   the state index in [0, S) of every row: one int for all rows, or one per row; None: 0.  The rows of a
                stream are its consecutive frames in row order (and from call to call)
      settings  the keys of TRACKER (track_settings); max_tracks must be the state's
      association  "greedy": the three greedy associations of codetr_hip.h; "optimal": each association is an assignment
                problem over integer gains, solved in the same launch (codetr_track_update2_*; the rule is stated in
                include/codetr_assign.h).  The state is the same: a stream may switch between calls
      motion    None, or estimate_motion's [N, 4] float32 (dx, dy, valid, 0 per row) on the detections' device: a valid,
                finite motion is added to the predicted centres of the row's live tracks before association
                (codetr_track_update3_*, include/codetr_motion.h).  None calls exactly the entry points it always did.
                Or estimate_motion(model="similarity")'s [N, 8] float32: by the row's model the similarity moves the
                predicted centres, their velocities and the height, or the translation is added (codetr_track_update4_*)
      appearance  None, or appearance_descriptors' [N, Q, 128] int16 of these detections: the first two associations add
                the colour similarity of track and candidate to the pair value, and a lost track inside the gate can match
                on it alone (codetr_track_update5_*, include/codetr_appearance.h).  A [N, 4] motion is widened on the
                device to [N, 8] with model = valid.  None calls exactly the entry points it always did.
      appearance_state     new_appearance_state's tensor for the same streams and max_tracks, updated in place; given
                exactly when `appearance` is
      appearance_settings  the keys of APPEARANCE (appearance_settings)
    -> [N, Q] int32 on the device: the id of the track each row updated or started, negated while the track is
    tentative, 0 for no track and beyond count."""
    cfg = track_settings(settings)
    if not isinstance(association, str) or association not in _assign.ASSOCIATIONS:
        raise ValueError(f"track_update: association must be one of {list(TRACK_ASSOCIATIONS)}, got {association!r}")
    scores = dets.scores
    _gpu(scores, "track_update")
    T = _track_slots(state)
    if state.device != scores.device:
        raise ValueError("track_update: the state lives on another device than the detections")
    if settings is not None and "max_tracks" in settings and cfg["max_tracks"] != T:
        raise ValueError(f"track_update: max_tracks {cfg['max_tracks']} but the state has {T} slots")
    N, Q = _check.detections("track_update", dets, scores.device, _cabi.POSTPROCESS_MAX_Q)
    if motion is not None:
        if not torch.is_tensor(motion) or motion.dtype != torch.float32 or \
                tuple(motion.shape) not in ((N, 4), (N, 8)) or motion.device != scores.device:
            raise ValueError("track_update: motion must be a [N, 4] or [N, 8] float32 tensor on the detections' device")
        motion = motion.contiguous()
    if (appearance is None) != (appearance_state is None):
        raise ValueError("track_update: appearance and appearance_state go together (appearance_descriptors, "
                         "new_appearance_state)")
    app_cfg = None
    if appearance is not None:
        app_cfg = _appearance_settings(appearance_settings)
        if not torch.is_tensor(appearance) or appearance.dtype != torch.int16 or \
                tuple(appearance.shape) != (N, Q, _appearance.BINS) or appearance.device != scores.device:
            raise ValueError(f"track_update: appearance must be a [N, Q, {_appearance.BINS}] int16 tensor on the "
                             "detections' device (appearance_descriptors)")
        if not torch.is_tensor(appearance_state) or appearance_state.dtype != torch.int16 or \
                appearance_state.dim() != 3 or not appearance_state.is_contiguous() or \
                appearance_state.device != scores.device or \
                tuple(appearance_state.shape) != (state.shape[0], T, _appearance.BINS):
            raise ValueError(f"track_update: appearance_state must be a contiguous [{state.shape[0]}, {T}, "
                             f"{_appearance.BINS}] int16 tensor on the detections' device (new_appearance_state)")
        appearance = appearance.contiguous()
        if motion is not None and motion.shape[1] == 4:   # model = valid: 1.0 adds the translation, 0.0 nothing
            motion = torch.cat([motion[:, :3], motion[:, 2:3], torch.zeros_like(motion)], dim=1).contiguous()
    streams = track_streams(streams, N)
    if any(v >= state.shape[0] for v in streams):
        raise ValueError(f"track_update: a stream index outside the state's {state.shape[0]} streams")
    ids = torch.zeros((N, Q), dtype=torch.int32, device=scores.device) if N == 0 or Q == 0 else \
        torch.empty((N, Q), dtype=torch.int32, device=scores.device)
    if N == 0 or Q == 0:
        return ids
    boxes, scores = dets.boxes.contiguous(), scores.contiguous()
    labels, count = dets.labels.contiguous(), dets.count.contiguous()
    thr = (cfg["obj_score_thrs"]["high"], cfg["obj_score_thrs"]["low"], cfg["init_track_thr"],
           cfg["match_iou_thrs"]["high"], cfg["match_iou_thrs"]["low"], cfg["match_iou_thrs"]["tentative"])
    with torch.cuda.device(scores.device):
        work = None
        if appearance is not None:
            work = torch.empty((_appearance.work_bytes(state.shape[0], T, Q),), dtype=torch.uint8, device=scores.device)
        for i, j in _check.chunks(N):
            args = (boxes[i:j], scores[i:j], labels[i:j], count[i:j], streams[i:j], state, T, thr,
                    cfg["num_frames_retain"], cfg["num_tentatives"], cfg["weight_iou_with_det_scores"], ids[i:j])
            if appearance is not None:
                _appearance.track_update5(*args, _assign.ASSOCIATIONS[association], None if motion is None else motion[i:j],
                                          appearance[i:j], appearance_state,
                                          (app_cfg["appearance_thr"], app_cfg["proximity_thr"], app_cfg["reid_gate"]), work)
            elif motion is not None and motion.shape[1] == 8:
                _motion.track_update4(*args, _assign.ASSOCIATIONS[association], motion[i:j])
            elif motion is not None:
                _motion.track_update3(*args, _assign.ASSOCIATIONS[association], motion[i:j])
            elif association == "greedy":
                _cabi.track_update(*args)
            else:
                _assign.track_update2(*args, _assign.ASSOCIATIONS[association])
    return ids


# camera-motion compensation (include/codetr_motion.h states the rule and these settings' ranges)
MOTION = dict(grid=_motion.GRID_MAX, search=8, texture=2, min_blocks=4)
MOTION_MODELS = ("translation", "similarity")
MotionState = collections.namedtuple("MotionState", "have H W k thumb")


def motion_settings(d=None):
    """the settings of estimate_motion, validated and completed from MOTION -> a new dict.  ValueError for an unknown key or
    a value that is not an integer of its range: grid 32..160, search 1..16, texture 0..65535, min_blocks 1..100."""
    return _check.validated("motion", MOTION, d, dict(
        grid=_check.whole(_motion.GRID_MIN, _motion.GRID_MAX), search=_check.whole(1, _motion.SEARCH_MAX),
        texture=_check.whole(0, _motion.TEXTURE_MAX), min_blocks=_check.whole(1, _motion.MAX_BLOCKS)))


def new_motion_state(S, device):
    """the motion states of S fresh streams: zeros [S, 16 + 160 * 160] uint8 on `device` (int32 have, H, W, k, then the
    stream's last thumbnail; motion_state_to_host decodes it)"""
    if int(S) < 1:
        raise ValueError(f"new_motion_state: at least one stream, got {S}")
    return torch.zeros((int(S), _motion.state_bytes()), dtype=torch.uint8, device=device)


def motion_state_to_host(state):
    """the states of new_motion_state / estimate_motion on the host (one device-to-host copy) -> MotionState of numpy
    arrays: have, H, W, k [S] int32 and thumb [S, 160 * 160] uint8 (rows at pitch W // k, zero behind them)"""
    raw = state.cpu().numpy()
    hdr = raw[:, :16].copy().view(np.int32)
    return MotionState(hdr[:, 0].copy(), hdr[:, 1].copy(), hdr[:, 2].copy(), hdr[:, 3].copy(), raw[:, 16:].copy())


def estimate_motion(src_u8, rows, state, streams=None, settings=None, model="translation"):
    """The global image motion between the consecutive frames of every stream, in three launches per
    PREPROCESS_BATCH_MAX images and without a synchronisation (csrc/motion.hip; include/codetr_motion.h states the rule:
    block matching of gray thumbnails, a median vote, translation only).  model="similarity": five launches, the same
    votes fitted with a zoom and a roll as well (the header's version 2); the state is the same, so a stream may switch
    between the models from call to call.
      src_u8    one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows      (offset, H, W) per image
      state     new_motion_state's tensor, updated in place: it keeps every stream's last thumbnail between calls
      streams   the state index in [0, S) of every row, as track_update's
      settings  the keys of MOTION (motion_settings)
    -> (motion [N, 4] float32: dx, dy, valid (1.0 / 0.0), 0 -- scene content at p in the previous frame of the stream is
    at p + (dx, dy) in this one, in source pixels; diag [N, 4] int32: k, blocks, textured, agreeing), on the device.
    model="similarity" -> (motion [N, 8] float32: dx, dy, valid, model (2.0 similarity, 1.0 translation, 0.0 none), a, b,
    px, py -- content at p is at (px + dx, py + dy) + [[a, -b], [b, a]] (p - (px, py)); diag [N, 8] int32: the four above,
    eligible pairs, the best pair's inliers, its i, its j)."""
    if model not in MOTION_MODELS:
        raise ValueError(f"estimate_motion: model must be one of {list(MOTION_MODELS)}, got {model!r}")
    sim = model == "similarity"
    cfg = motion_settings(settings)
    _gpu(src_u8, "estimate_motion")
    rows = _check.image_rows("estimate_motion", src_u8, rows, _cabi.FRAME_MAX_SIDE)
    if not torch.is_tensor(state) or state.dtype != torch.uint8 or state.dim() != 2 or not state.is_contiguous() or \
            state.shape[0] < 1 or state.shape[1] != _motion.state_bytes():
        raise ValueError("estimate_motion: the state is a contiguous [S, 16 + 160 * 160] uint8 tensor (new_motion_state)")
    if state.device != src_u8.device:
        raise ValueError("estimate_motion: the state lives on another device than the images")
    N = len(rows)
    streams = track_streams(streams, N)
    if any(v >= state.shape[0] for v in streams):
        raise ValueError(f"estimate_motion: a stream index outside the state's {state.shape[0]} streams")
    motion = torch.empty((N, 8 if sim else 4), dtype=torch.float32, device=src_u8.device)
    diag = torch.empty((N, 8 if sim else 4), dtype=torch.int32, device=src_u8.device)
    four = (cfg["grid"], cfg["search"], cfg["texture"], cfg["min_blocks"])
    with torch.cuda.device(src_u8.device):
        for i, j in _check.chunks(N):
            nbytes = _motion.work2_bytes(j - i) if sim else _motion.work_bytes(j - i)
            work = torch.empty((nbytes,), dtype=torch.uint8, device=src_u8.device)
            if sim:
                _motion.estimate(src_u8, rows[i:j], streams[i:j], state, four, work, motion[i:j], diag[i:j], similarity=True)
            else:
                _motion.estimate(src_u8, rows[i:j], streams[i:j], state, four, work, motion[i:j], diag[i:j])
    return motion, diag


ASSIGN_MAX_ROWS, ASSIGN_MAX_COLS, ASSIGN_MAX_GAIN = _assign.MAX_ROWS, _assign.MAX_COLS, _assign.MAX_GAIN


def linear_assignment(gain):
    """Maximum-weight assignment of integer gains on the GPU, one workgroup per problem in one launch (csrc/assign.hip;
    the procedure and its tie rule are stated in include/codetr_assign.h, so the matches -- not just their total -- are
    reproducible): the shape of a DETR matcher, up to 512 targets x 1024 queries, after the caller has turned its costs
    into gains.
      gain  [n, m] or [B, n, m] int32 on a GPU, n <= ASSIGN_MAX_ROWS, m <= ASSIGN_MAX_COLS; values are clamped into
            [0, ASSIGN_MAX_GAIN]; a pair of gain 0 is never matched
    -> (match [.., n] int32: the column of every row, -1 for unmatched; total [..] int64: the sum of the matched gains)"""
    if not torch.is_tensor(gain) or gain.dtype != torch.int32 or gain.dim() not in (2, 3):
        raise ValueError("linear_assignment: gain must be an int32 tensor [n, m] or [B, n, m]")
    B, n, m = gain.shape if gain.dim() == 3 else (1,) + tuple(gain.shape)
    if n > ASSIGN_MAX_ROWS or m > ASSIGN_MAX_COLS:
        raise ValueError(f"linear_assignment: at most {ASSIGN_MAX_ROWS} rows x {ASSIGN_MAX_COLS} columns, got {n} x {m}")
    _gpu(gain, "linear_assignment")
    g = gain.contiguous().view(B, n, m)
    match = torch.full((B, n), -1, dtype=torch.int32, device=g.device)
    total = torch.zeros((B,), dtype=torch.int64, device=g.device)
    if B and n and m:
        with torch.cuda.device(g.device):
            for i in range(0, B, 65535):
                _assign.assign(g[i:i + 65535], match[i:i + 65535], total[i:i + 65535])
    return (match, total) if gain.dim() == 3 else (match[0], total[0])


def track_streams(streams, N):
    """the `streams` argument of track_update and Inferencer.__call__ -> a list of N non-negative ints: None is stream 0
    for every row, one int is that stream for every row; ValueError for anything else"""
    def one(v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"streams: non-negative integers, got {v!r}")
        return int(v)

    if streams is None:
        return [0] * N
    if isinstance(streams, (int, np.integer)):
        return [one(streams)] * N
    if not isinstance(streams, (list, tuple, np.ndarray)) or len(streams) != N:
        raise ValueError(f"streams: one non-negative integer, or one per frame ({N})")
    return [one(v) for v in streams]
