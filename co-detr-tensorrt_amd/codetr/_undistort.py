"""ctypes binding of the lens-undistortion entry points of libcodetr_hip.so (C ABI: include/codetr_undistort.h, a companion
header of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures and the
CODETR_UNDISTORT_* constants are read from it by _cabi.companion, and a library that lacks an entry point is an
ImportError.
"""
import ctypes

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_undistort.h", "undistort", "undistortion")

ABI_VERSION = defines["CODETR_UNDISTORT_ABI_VERSION"]
ROW_INTS = defines["CODETR_UNDISTORT_ROW_INTS"]
PARAM_FLOATS = defines["CODETR_UNDISTORT_PARAM_FLOATS"]
MAX_FOCAL = defines["CODETR_UNDISTORT_MAX_FOCAL"]
MAX_CENTRE = defines["CODETR_UNDISTORT_MAX_CENTRE"]
MODELS = {n.lower(): defines["CODETR_UNDISTORT_" + n] for n in ("BROWN", "FISHEYE")}

_cabi.CALLS.setdefault("undistort", 0)


def remap(src, rows, params, dst):
    """src: flat uint8 device buffer, only read; rows: <= PREPROCESS_BATCH_MAX (model code, H, W, src offset, src pitch, H',
    W', dst offset, fill 0xRRGGBB); params: per row the sixteen fp32 parameters; dst: another flat uint8 buffer on src's
    device (include/codetr_undistort.h states the rule)"""
    _cabi.CALLS["undistort"] += 1
    rc = load().codetr_undistort_rgb_u8(_cabi.current_stream_ptr(src.device), src.data_ptr(), src.numel(), len(rows),
                                        (ctypes.c_int64 * (ROW_INTS * len(rows)))(*[int(v) for r in rows for v in r]),
                                        (ctypes.c_float * (PARAM_FLOATS * len(rows)))(*[v for p in params for v in p]),
                                        dst.data_ptr(), dst.numel())
    _cabi.check(rc, "codetr_undistort_rgb_u8")
