"""The tracker's output on the picture (hip_ops re-exports these names): the history of every track's position, kept on the
device, and the drawing of trails, per-identity colours and ids on the chunk's images.  GPU-only, as hip_ops;
include/codetr_draw_tracks.h states the rule and its limits, csrc/draw_tracks.hip holds the kernels.  (A module of its own,
as crop_ops: it draws with image_ops' tables and style and walks streams as track_ops does.)
"""
import torch

from . import _cabi, _draw_tracks
from . import _operands as _check
from ._operands import _gpu
from .image_ops import DRAW_NAME_ROW, DRAW_STYLE, draw_style
from .track_ops import TRACKER, TRACK_MAX_TRACKS, track_streams

__all__ = ["TRAILS", "TRAIL_ANCHORS", "TRAIL_COLOR_BY", "TRAIL_MAX_LENGTH", "trail_settings", "new_trail_state",
           "trail_snapshot_bytes", "trail_update", "draw_tracks"]

# trail: points per track, 0 = no trails; retain: frames an unseen track keeps its trail (the tracker's num_frames_retain)
TRAILS = dict(color_by="track", show_id=True, trail=30, trail_width=2, trail_alpha=0.6, anchor="center", tentative=False,
              untracked=True, retain=TRACKER["num_frames_retain"])
TRAIL_ANCHORS = tuple(_draw_tracks.ANCHORS)
TRAIL_COLOR_BY = tuple(_draw_tracks.COLOR_BY)
TRAIL_MAX_LENGTH = _draw_tracks.MAX_LENGTH


def _length(v):
    if v != 0:
        try:
            return _check.whole(_draw_tracks.MIN_LENGTH, _draw_tracks.MAX_LENGTH)(v)
        except _check._Not:
            raise _check._Not(f"0 (no trails) or an integer in {_draw_tracks.MIN_LENGTH}..{_draw_tracks.MAX_LENGTH}") from None
    return _check.whole(0, 0)(v)


def trail_settings(settings=None):
    """the settings of trail_update and draw_tracks, validated and completed from TRAILS -> a new dict.  ValueError, naming
    the key, for an unknown key, a color_by outside TRAIL_COLOR_BY, an anchor outside TRAIL_ANCHORS, a trail that is not 0
    or 2..64, a trail_width outside 1..15, a trail_alpha outside [0, 1], a retain < 1, a switch that is not a bool."""
    def switch(v):
        if not isinstance(v, bool):
            raise _check._Not("True or False")
        return v

    return _check.validated("tracks", TRAILS, settings, dict(
        color_by=_check.one_of(TRAIL_COLOR_BY), anchor=_check.one_of(TRAIL_ANCHORS), trail=_length,
        trail_width=_check.whole(1, 15), trail_alpha=_check.number(0, 1), retain=_check.whole(1, 2 ** 31 - 1),
        show_id=switch, tentative=switch, untracked=switch), sep=": ")


def _shape(name, max_tracks, length):
    if not 1 <= int(max_tracks) <= TRACK_MAX_TRACKS:
        raise ValueError(f"{name}: max_tracks in 1..{TRACK_MAX_TRACKS}, got {max_tracks}")
    if not _draw_tracks.MIN_LENGTH <= int(length) <= _draw_tracks.MAX_LENGTH:
        raise ValueError(f"{name}: length in {_draw_tracks.MIN_LENGTH}..{_draw_tracks.MAX_LENGTH}, got {length}")


def new_trail_state(S, max_tracks, length, device):
    """the trail states of S fresh streams, max_tracks entries of `length` points each: zeros
    [S, 16 + 16 max_tracks + 4 max_tracks length] uint8 on `device` (include/codetr_draw_tracks.h states the layout)"""
    if int(S) < 1:
        raise ValueError(f"new_trail_state: at least one stream, got {S}")
    _shape("new_trail_state", max_tracks, length)
    return torch.zeros((int(S), _draw_tracks.state_bytes(max_tracks, length)), dtype=torch.uint8, device=device)


def trail_snapshot_bytes(max_tracks, length):
    """bytes of one row of trail_update's result (host only)"""
    _shape("trail_snapshot_bytes", max_tracks, length)
    return _draw_tracks.snapshot_bytes(max_tracks, length)


def _entries(name, t, length, head, what):
    """the max_tracks of a [rows, head + (16 + 4 length) max_tracks] uint8 tensor"""
    per = 16 + 4 * length
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous() or \
            t.shape[1] <= head or (t.shape[1] - head) % per or (t.shape[1] - head) // per > TRACK_MAX_TRACKS:
        raise ValueError(f"{name}: {what} must be a contiguous [rows, {head} + {per} max_tracks] uint8 tensor for trails of "
                         f"{length} points")
    return (t.shape[1] - head) // per


def _ids(name, track_ids, scores):
    if not torch.is_tensor(track_ids) or track_ids.dtype != torch.int32 or track_ids.device != scores.device or \
            tuple(track_ids.shape) != tuple(scores.shape):
        raise ValueError(f"{name}: track_ids must be a [N, Q] int32 tensor on the detections' device (track_update's result)")
    return track_ids.contiguous()


def trail_update(dets, track_ids, state, streams=None, settings=None):
    """The trails of a chunk's frames in one launch per PREPROCESS_BATCH_MAX rows and without a synchronisation
    (trail_update_kernel in csrc/draw_tracks.hip; include/codetr_draw_tracks.h states the rule): per frame of a stream, in
    row order, unseen tracks are retired, every tracked detection appends its anchor point to the ring of its id, new ids
    take the free entries, and the row's snapshot is written.
      dets       Detections / SoftDetections over [N, Q] rows, Q <= 1024 (boxes and count are read)
      track_ids  track_update's [N, Q] int32 for these detections
      state      new_trail_state's tensor, updated in place; it stays on the device between calls
      streams    the state index in [0, S) of every row, as track_update's
      settings   the keys of TRAILS (trail_settings); `trail` must be the state's length, and not 0
    -> [N, trail_snapshot_bytes] uint8 on the device: per row what draw_tracks draws for that frame."""
    cfg = trail_settings(settings)
    K = cfg["trail"]
    if K == 0:
        raise ValueError("trail_update: trail = 0 means no trails; nothing to update")
    scores = dets.scores
    _gpu(scores, "trail_update")
    N, Q = _check.detections("trail_update", dets, scores.device, _cabi.POSTPROCESS_MAX_Q)
    T = _entries("trail_update", state, K, 16, "the state (new_trail_state)")
    if state.device != scores.device:
        raise ValueError("trail_update: the state lives on another device than the detections")
    ids = _ids("trail_update", track_ids, scores)
    streams = track_streams(streams, N)
    if any(v >= state.shape[0] for v in streams):
        raise ValueError(f"trail_update: a stream index outside the state's {state.shape[0]} streams")
    out = torch.empty((N, _draw_tracks.snapshot_bytes(T, K)), dtype=torch.uint8, device=scores.device)
    if N == 0 or Q == 0:
        return out.zero_()
    boxes, count = dets.boxes.contiguous(), dets.count.contiguous()
    with torch.cuda.device(scores.device):
        for i, j in _check.chunks(N):
            _draw_tracks.trail_update(boxes[i:j], count[i:j], streams[i:j], state, T, K, ids[i:j], cfg["retain"],
                                      _draw_tracks.ANCHORS[cfg["anchor"]], cfg["tentative"], out[i:j])
    return out


def draw_tracks(buf_u8, rows, dets, track_ids, trails, names, palette, track_palette, style=None):
    """draw_detections for tracked detections, in one launch per PREPROCESS_BATCH_MAX images (draw_tracks_kernel in
    csrc/draw_tracks.hip; include/codetr_draw_tracks.h states the rendering): first the trails, each blended once per
    pixel in the colour of its id; then the outlines, in the id's colour under color_by="track"; then the labels, as
    "#<id> <name>: <percent>" under show_id ('~' for a tentative track).  In place.
      buf_u8, rows, dets, names, palette   as draw_detections', Q <= 1024
      track_ids      track_update's [N, Q] int32 for these detections
      trails         trail_update's [N, trail_snapshot_bytes] uint8 for these rows, or None: no trails
      track_palette  [P, 3] uint8 on the device: identity i takes colour (i - 1) % P
      style          the keys of DRAW_STYLE and of TRAILS (`trail` must be the snapshots' length; `anchor`, `tentative`
                     and `retain` are trail_update's and not read here)
    -> buf_u8.  ValueError for Q > 1024, a bad style value, a wrong dtype or shape, CPU tensors.  With every id 0,
    untracked=True and no trails the bytes are draw_detections'.  Nothing is launched when N == 0 or Q == 0."""
    style = dict(style or {})
    st = draw_style({k: v for k, v in style.items() if k in DRAW_STYLE})
    ts = trail_settings({k: v for k, v in style.items() if k not in DRAW_STYLE})
    rows = _check.image_rows("draw_tracks", buf_u8, rows, _cabi.DRAW_MAX_SIDE)
    _check.same_gpu("draw_tracks", buf_u8.device, names=names, palette=palette, track_palette=track_palette)
    C = palette.shape[0] if palette.dim() == 2 else 0
    if names.dtype != torch.uint8 or palette.dtype != torch.uint8 or C == 0 or tuple(palette.shape) != (C, 3) or \
            tuple(names.shape) != (C, DRAW_NAME_ROW):
        raise ValueError("draw_tracks: names [C, 24] and palette [C, 3] in uint8, C > 0")
    if track_palette.dtype != torch.uint8 or track_palette.dim() != 2 or track_palette.shape[1] != 3 or \
            not 1 <= track_palette.shape[0] <= 65536:
        raise ValueError("draw_tracks: track_palette [P, 3] in uint8, P in 1..65536")
    N, Q = _check.detections("draw_tracks", dets, buf_u8.device, _cabi.POSTPROCESS_MAX_Q, len(rows))
    ids = _ids("draw_tracks", track_ids, dets.scores)
    T = 0
    if trails is not None:
        _check.same_gpu("draw_tracks", buf_u8.device, trails=trails)
        if ts["trail"] == 0:
            raise ValueError("draw_tracks: trail = 0 means no trails: pass trails=None")
        T = _entries("draw_tracks", trails, ts["trail"], 0, "trails (trail_update's result)")
        if trails.shape[0] != N:
            raise ValueError(f"draw_tracks: one snapshot per image ({N}), got {trails.shape[0]}")
    if N == 0 or Q == 0:
        return buf_u8
    boxes, scores, labels, count = (t.contiguous() for t in (dets.boxes, dets.scores, dets.labels, dets.count))
    tc = st["text_color"]
    with torch.cuda.device(buf_u8.device):
        for i, j in _check.chunks(N):
            _draw_tracks.draw_tracks(buf_u8, rows[i:j], boxes[i:j], scores[i:j], labels[i:j], count[i:j],
                                     palette.contiguous(), names.contiguous(), st["line_width"], st["alpha"],
                                     st["score_thr"], (tc[0] << 16) | (tc[1] << 8) | tc[2], st["font_scale"],
                                     st["draw_labels"], ids[i:j], None if trails is None else trails[i:j], T, ts["trail"],
                                     track_palette.contiguous(), ts["trail_width"], ts["trail_alpha"],
                                     _draw_tracks.COLOR_BY[ts["color_by"]], ts["show_id"], ts["untracked"])
    return buf_u8
