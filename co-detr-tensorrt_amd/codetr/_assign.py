"""ctypes binding of the assignment entry points of libcodetr_hip.so (C ABI: include/codetr_assign.h, a companion
header of codetr_hip.h with a version of its own).  As in _jpeg.py the header is the one written copy: the signatures
and the CODETR_ASSIGN_* / CODETR_ASSOCIATION_* constants are read from it with _cheader.parse, and a library that lacks
an entry point is an ImportError.
"""
import os

from . import _cabi, _cheader

HEADER_PATH = os.path.join(os.path.dirname(_cheader.HEADER_PATH), "codetr_assign.h")
if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the assignment binding is derived from it")
with open(HEADER_PATH) as _f:
    functions, defines = _cheader.parse(_f.read())

ABI_VERSION = defines["CODETR_ASSIGN_ABI_VERSION"]
MAX_ROWS = defines["CODETR_ASSIGN_MAX_ROWS"]
MAX_COLS = defines["CODETR_ASSIGN_MAX_COLS"]
MAX_GAIN = defines["CODETR_ASSIGN_MAX_GAIN"]
ASSOCIATIONS = {"greedy": defines["CODETR_ASSOCIATION_GREEDY"], "optimal": defines["CODETR_ASSOCIATION_OPTIMAL"]}

SIGNATURES = {name: (_cabi._CTYPE[_cheader.kind(ret, returned=True)], [_cabi._CTYPE[_cheader.kind(t)] for t, _ in params])
              for name, (ret, params) in functions.items()}

_cabi.CALLS.setdefault("assign", 0)
_cabi.CALLS.setdefault("track_update2", 0)
_lib = None


def load():
    """the shared library with the assignment prototypes set; ImportError when it is absent or older than this header"""
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
    ver = lib.codetr_assign_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"{_cabi.LIB_PATH} has assignment ABI version {ver}, host expects {ABI_VERSION}; rebuild the extension")
    _lib = lib
    return lib


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
