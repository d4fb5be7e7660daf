"""ctypes binding of the track-drawing entry points of libcodetr_hip.so (C ABI: include/codetr_draw_tracks.h, a companion
header of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures and the
CODETR_TRAIL_* / CODETR_COLOR_BY_* constants are read from it by _cabi.companion, and a library that lacks an entry point
is an ImportError.
"""
import ctypes

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_draw_tracks.h", "draw_tracks", "track drawing")

ABI_VERSION = defines["CODETR_DRAW_TRACKS_ABI_VERSION"]
MIN_LENGTH, MAX_LENGTH = defines["CODETR_TRAIL_MIN_LENGTH"], defines["CODETR_TRAIL_MAX_LENGTH"]
ANCHORS = {name: defines["CODETR_TRAIL_" + name.upper()] for name in ("center", "bottom")}
COLOR_BY = {name: defines["CODETR_COLOR_BY_" + name.upper()] for name in ("class", "track")}

_cabi.CALLS.setdefault("trail_update", 0)
_cabi.CALLS.setdefault("draw_tracks", 0)


def _sized(fn, max_tracks, length):
    n = int(getattr(load(), fn)(int(max_tracks), int(length)))
    if n < 0:
        _cabi.check(n, fn)
    return n


def state_bytes(max_tracks, length):
    """bytes of one stream's trail state (host only, no GPU); the header states the layout"""
    return _sized("codetr_trail_state_bytes", max_tracks, length)


def snapshot_bytes(max_tracks, length):
    """bytes of one row's snapshot, what draw_tracks reads (host only, no GPU)"""
    return _sized("codetr_trail_snapshot_bytes", max_tracks, length)


def trail_update(boxes, count, streams, state, max_tracks, length, ids, retain, anchor, tentative, out):
    """boxes [N, Q, 4] in f16 / bf16 / f32, count [N] int32, N <= PREPROCESS_BATCH_MAX; streams: the state index of every
    row; state [S, state_bytes] uint8, updated in place; ids [N, Q] int32 as track_update wrote them; anchor: a value of
    ANCHORS; out [N, snapshot_bytes] uint8 (include/codetr_draw_tracks.h states the rule)"""
    _cabi.CALLS["trail_update"] += 1
    N, Q = ids.shape
    name = "codetr_trail_update_" + _cabi._SUFFIX[boxes.dtype]
    rc = getattr(load(), name)(
        _cabi.current_stream_ptr(boxes.device), boxes.data_ptr(), None, None, count.data_ptr(), N, Q,
        (ctypes.c_int * N)(*[int(v) for v in streams]), state.shape[0], state.data_ptr(), int(max_tracks), int(length),
        ids.data_ptr(), int(retain), int(anchor), 1 if tentative else 0, out.data_ptr())
    _cabi.check(rc, name)


def draw_tracks(buf, rows, boxes, scores, labels, count, palette, names, line_width, alpha, score_thr, text_rgb,
                font_scale, draw_labels, ids, trails, max_tracks, length, track_palette, trail_width, trail_alpha, color_by,
                show_id, untracked):
    """_cabi.draw_detections' operands, then ids [N, Q] int32, trails [N, snapshot_bytes] uint8 or None (no trails) with
    its max_tracks and length, track_palette [P, 3] uint8 on the device, and the style (color_by: a value of COLOR_BY)"""
    _cabi.CALLS["draw_tracks"] += 1
    N, Q = scores.shape
    name = "codetr_draw_tracks_" + _cabi._SUFFIX[scores.dtype]
    rc = getattr(load(), name)(
        _cabi.current_stream_ptr(buf.device), buf.data_ptr(), buf.numel(), N,
        (ctypes.c_int64 * (3 * N))(*[int(v) for row in rows for v in row]), boxes.data_ptr(), scores.data_ptr(),
        labels.data_ptr(), count.data_ptr(), Q, palette.data_ptr(), names.data_ptr(), palette.shape[0], int(line_width),
        float(alpha), float(score_thr), int(text_rgb), int(font_scale), 1 if draw_labels else 0, ids.data_ptr(),
        _cabi._ptr(trails), int(max_tracks), int(length), track_palette.data_ptr(), track_palette.shape[0],
        int(trail_width), float(trail_alpha), int(color_by), 1 if show_id else 0, 1 if untracked else 0)
    _cabi.check(rc, name)
