"""ctypes binding of the appearance entry points of libcodetr_hip.so (C ABI: include/codetr_appearance.h, a companion
header of codetr_hip.h with a version of its own).  As in _motion.py the header is the one written copy: the signatures
and the CODETR_APPEARANCE_* constants are read from it with _cheader.parse, and a library that lacks an entry point is an
ImportError.
"""
import ctypes
import os

from . import _cabi, _cheader

HEADER_PATH = os.path.join(os.path.dirname(_cheader.HEADER_PATH), "codetr_appearance.h")
if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the appearance binding is derived from it")
with open(HEADER_PATH) as _f:
    functions, defines = _cheader.parse(_f.read())

ABI_VERSION = defines["CODETR_APPEARANCE_ABI_VERSION"]
BINS = defines["CODETR_APPEARANCE_BINS"]
COLS, ROWS = defines["CODETR_APPEARANCE_COLS"], defines["CODETR_APPEARANCE_ROWS"]

SIGNATURES = {name: (_cabi._CTYPE[_cheader.kind(ret, returned=True)], [_cabi._CTYPE[_cheader.kind(t)] for t, _ in params])
              for name, (ret, params) in functions.items()}

_cabi.CALLS.setdefault("appearance_describe", 0)
_cabi.CALLS.setdefault("track_update5", 0)
_lib = None


def load():
    """the shared library with the appearance prototypes set; ImportError when it is absent or older than this header"""
    global _lib
    if _lib is not None:
        return _lib
    _cabi.load()
    lib = _cabi._lib   # (the plain library: these entries are not part of a launch plan and are never recorded)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{_cabi.LIB_PATH} does not export {name}; rebuild the extension") from e
        fn.restype = res
        fn.argtypes = args
    ver = lib.codetr_appearance_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"{_cabi.LIB_PATH} has appearance ABI version {ver}, host expects {ABI_VERSION}; rebuild the "
                          "extension")
    _lib = lib
    return lib


def state_bytes(max_tracks):
    return int(load().codetr_appearance_state_bytes(int(max_tracks)))


def work_bytes(S, max_tracks, Q):
    return int(load().codetr_appearance_work_bytes(int(S), int(max_tracks), int(Q)))


def describe(src, rows, boxes, count, desc_out):
    """src flat uint8, rows [(offset, H, W)] of N images, boxes [N, Q, 4] f16 / bf16 / f32, count [N] int32, desc_out
    [N, Q, 128] int16 (the uint16 bits), all contiguous on one device (include/codetr_appearance.h)"""
    _cabi.CALLS["appearance_describe"] += 1
    N, Q = boxes.shape[0], boxes.shape[1]
    name = "codetr_appearance_describe_" + _cabi._SUFFIX[boxes.dtype]
    flat = [int(v) for r in rows for v in r]
    rc = getattr(load(), name)(
        _cabi.current_stream_ptr(src.device), src.data_ptr(), src.numel(), N, (ctypes.c_int64 * (3 * len(rows)))(*flat),
        boxes.data_ptr(), count.data_ptr(), Q, desc_out.data_ptr())
    _cabi.check(rc, name)


def track_update5(boxes, scores, labels, count, streams, state, max_tracks, thresholds, retain, tentatives, weight_iou,
                  ids_out, association, motion, desc, app_state, app_settings, work):
    """_motion.track_update4's arguments (motion [N, 8] float32 or None) + desc [N, Q, 128] int16 or None, app_state
    [S, T, 128] int16, app_settings (appearance_thr, proximity_thr, reid_gate), work uint8 of work_bytes(S, T, Q)
    -> codetr_track_update5_*"""
    _cabi.CALLS["track_update5"] += 1
    name = "codetr_track_update5_" + _cabi._SUFFIX[scores.dtype]
    _cabi._track_call(getattr(load(), name), name, boxes, scores, labels, count, streams, state, max_tracks, thresholds,
                      retain, tentatives, weight_iou, ids_out, int(association), _cabi._ptr(motion), _cabi._ptr(desc),
                      _cabi._ptr(app_state),
                      None if app_settings is None else (ctypes.c_float * 3)(*[float(v) for v in app_settings]),
                      _cabi._ptr(work), 0 if work is None else work.numel())
