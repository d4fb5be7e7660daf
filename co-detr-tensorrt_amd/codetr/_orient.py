"""ctypes binding of the orientation entry points of libcodetr_hip.so (C ABI: include/codetr_orient.h, a companion header
of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures and the CODETR_ORIENT_*
constants are read from it by _cabi.companion, and a library that lacks an entry point is an ImportError.
"""
import ctypes

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_orient.h", "orient", "orientation")

ABI_VERSION = defines["CODETR_ORIENT_ABI_VERSION"]
ROW_INTS = defines["CODETR_ORIENT_ROW_INTS"]

_cabi.CALLS.setdefault("orient", 0)


def exif(data) -> int:
    """data: the file as a contiguous 1-D uint8 numpy array -> its EXIF orientation 1..8 (1 when it names none); host
    only, no GPU"""
    o = load().codetr_orient_exif(data.ctypes.data, data.size)
    if o < 0:
        _cabi.check(o, "codetr_orient_exif")
    return o


def orient(src, rows, dst):
    """src: flat uint8 device buffer, only read; rows: <= PREPROCESS_BATCH_MAX (o, H, W, src offset, src pitch, dst
    offset); dst: another flat uint8 buffer on src's device (include/codetr_orient.h states the rule)"""
    _cabi.CALLS["orient"] += 1
    rc = load().codetr_orient_rgb_u8(_cabi.current_stream_ptr(src.device), src.data_ptr(), src.numel(), len(rows),
                                     (ctypes.c_int64 * (ROW_INTS * len(rows)))(*[int(v) for r in rows for v in r]),
                                     dst.data_ptr(), dst.numel())
    _cabi.check(rc, "codetr_orient_rgb_u8")
