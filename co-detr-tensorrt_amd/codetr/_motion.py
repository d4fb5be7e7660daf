"""ctypes binding of the camera-motion entry points of libcodetr_hip.so (C ABI: include/codetr_motion.h, a companion
header of codetr_hip.h with a version of its own).  As in _assign.py the header is the one written copy: the signatures
and the CODETR_MOTION_* constants are read from it with _cheader.parse, and a library that lacks an entry point is an
ImportError.
"""
import ctypes
import os

from . import _cabi, _cheader

HEADER_PATH = os.path.join(os.path.dirname(_cheader.HEADER_PATH), "codetr_motion.h")
if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the camera-motion binding is derived from it")
with open(HEADER_PATH) as _f:
    functions, defines = _cheader.parse(_f.read())

ABI_VERSION = defines["CODETR_MOTION_ABI_VERSION"]
GRID_MIN, GRID_MAX = defines["CODETR_MOTION_GRID_MIN"], defines["CODETR_MOTION_GRID_MAX"]
BLOCK = defines["CODETR_MOTION_BLOCK"]
SEARCH_MAX = defines["CODETR_MOTION_SEARCH_MAX"]
TEXTURE_MAX = defines["CODETR_MOTION_TEXTURE_MAX"]
MAX_BLOCKS = defines["CODETR_MOTION_MAX_BLOCKS"]

SIGNATURES = {name: (_cabi._CTYPE[_cheader.kind(ret, returned=True)], [_cabi._CTYPE[_cheader.kind(t)] for t, _ in params])
              for name, (ret, params) in functions.items()}

_cabi.CALLS.setdefault("motion_estimate", 0)
_cabi.CALLS.setdefault("track_update3", 0)
_cabi.CALLS.setdefault("motion_estimate2", 0)
_cabi.CALLS.setdefault("track_update4", 0)
_lib = None


def load():
    """the shared library with the camera-motion prototypes set; ImportError when it is absent or older than this header"""
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
    ver = lib.codetr_motion_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"{_cabi.LIB_PATH} has camera-motion ABI version {ver}, host expects {ABI_VERSION}; rebuild the "
                          "extension")
    _lib = lib
    return lib


def state_bytes():
    return int(load().codetr_motion_state_bytes())


def work_bytes(N):
    return int(load().codetr_motion_work_bytes(int(N)))


def work2_bytes(N):
    return int(load().codetr_motion_work2_bytes(int(N)))


def estimate(src, rows, streams, state, settings, work, motion_out, diag_out, similarity=False):
    """src flat uint8, rows [(offset, H, W)] of N images, streams N ints, state [S, state_bytes()] uint8, settings
    (grid, search, texture, min_blocks), work uint8 of work_bytes(N), motion_out [N, 4] float32, diag_out [N, 4] int32,
    all contiguous on one device (include/codetr_motion.h); similarity: codetr_motion_estimate2_u8 with work2_bytes(N) of
    work and [N, 8] outputs"""
    name = "codetr_motion_estimate2_u8" if similarity else "codetr_motion_estimate_u8"
    _cabi.CALLS["motion_estimate2" if similarity else "motion_estimate"] += 1
    N = len(rows)
    flat = [int(v) for r in rows for v in r]
    rc = getattr(load(), name)(
        _cabi.current_stream_ptr(src.device), src.data_ptr(), src.numel(), N, (ctypes.c_int64 * (3 * N))(*flat),
        (ctypes.c_int * N)(*[int(v) for v in streams]), state.shape[0], state.data_ptr(),
        (ctypes.c_int * 4)(*[int(v) for v in settings]), work.data_ptr(), work.numel(), motion_out.data_ptr(),
        diag_out.data_ptr())
    _cabi.check(rc, name)


def track_update3(boxes, scores, labels, count, streams, state, max_tracks, thresholds, retain, tentatives, weight_iou,
                  ids_out, association, motion, form=3):
    """_assign.track_update2's arguments + motion ([N, 4] float32 on the device, or None) -> codetr_track_update3_*;
    form=4: motion [N, 8] -> codetr_track_update4_*"""
    _cabi.CALLS[f"track_update{form}"] += 1
    name = f"codetr_track_update{form}_" + _cabi._SUFFIX[scores.dtype]
    _cabi._track_call(getattr(load(), name), name, boxes, scores, labels, count, streams, state, max_tracks, thresholds,
                      retain, tentatives, weight_iou, ids_out, int(association), _cabi._ptr(motion))


def track_update4(*args):
    """track_update3's arguments with motion [N, 8] float32 (estimate's similarity rows) -> codetr_track_update4_*"""
    track_update3(*args, form=4)
