"""ctypes binding of the assignment entry points of libcodetr_hip.so (C ABI: include/codetr_assign.h, a companion
header of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures
and the CODETR_ASSIGN_* / CODETR_ASSOCIATION_* constants are read from it by _cabi.companion, and a library that lacks
an entry point is an ImportError.
"""
from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_assign.h", "assign", "assignment")

ABI_VERSION = defines["CODETR_ASSIGN_ABI_VERSION"]
MAX_ROWS = defines["CODETR_ASSIGN_MAX_ROWS"]
MAX_COLS = defines["CODETR_ASSIGN_MAX_COLS"]
MAX_GAIN = defines["CODETR_ASSIGN_MAX_GAIN"]
ASSOCIATIONS = {"greedy": defines["CODETR_ASSOCIATION_GREEDY"], "optimal": defines["CODETR_ASSOCIATION_OPTIMAL"]}

_cabi.CALLS.setdefault("assign", 0)
_cabi.CALLS.setdefault("track_update2", 0)


def assign(gain, match, total):
    """gain [B, n, m] int32, match [B, n] int32, total [B] int64, contiguous on one device (include/codetr_assign.h)"""
    _cabi.CALLS["assign"] += 1
    B, n, m = gain.shape
    rc = load().codetr_assign_i32(_cabi.current_stream_ptr(gain.device), gain.data_ptr(), B, n, m, match.data_ptr(),
                                  total.data_ptr())
    _cabi.check(rc, "codetr_assign_i32")


def track_update2(boxes, scores, labels, count, streams, state, max_tracks, thresholds, retain, tentatives, weight_iou,
                  ids_out, association):
    """_cabi.track_update's arguments + association (a value of ASSOCIATIONS) -> codetr_track_update2_*"""
    _cabi.CALLS["track_update2"] += 1
    name = "codetr_track_update2_" + _cabi._SUFFIX[scores.dtype]
    _cabi._track_call(getattr(load(), name), name, boxes, scores, labels, count, streams, state, max_tracks, thresholds,
                      retain, tentatives, weight_iou, ids_out, int(association))
