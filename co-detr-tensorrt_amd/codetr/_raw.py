"""ctypes binding of the raw Bayer entry points of libcodetr_hip.so (C ABI: include/codetr_raw.h, a companion header of
codetr_hip.h with a version of its own).  The header is the one written copy: the signatures and the CODETR_RAW_*
constants are read from it by _cabi.companion, and a library that lacks an entry point is an ImportError.
"""
import ctypes

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_raw.h", "raw", "raw")

ABI_VERSION = defines["CODETR_RAW_ABI_VERSION"]
ROW_INTS = defines["CODETR_RAW_ROW_INTS"]
SETTING_INTS = defines["CODETR_RAW_SETTING_INTS"]
LUT_BYTES = defines["CODETR_RAW_LUT_BYTES"]
FORMATS = {"bayer_" + n.lower(): defines["CODETR_RAW_" + n] for n in ("RGGB", "GRBG", "GBRG", "BGGR")}
METHODS = {n.lower(): defines["CODETR_RAW_" + n] for n in ("MALVAR", "BILINEAR")}

_cabi.CALLS.setdefault("raw", 0)


def multipliers(black, white, gains):
    """the rule's step 1 on the host -> (m_red, m_green, m_blue), or None for settings the rule does not take (white <=
    black, a multiplier of 2**32 or more); no GPU"""
    m = (ctypes.c_int64 * 3)()
    rc = load().codetr_raw_multipliers(int(black), int(white), (ctypes.c_double * 3)(*[float(g) for g in gains]), m)
    return tuple(m) if rc == 0 else None


def to_rgb(src, rows, operands, lut, dst):
    """src: flat uint8 device buffer, only read; rows: <= PREPROCESS_BATCH_MAX (pattern code, bits, H, W, src offset, pitch,
    dst offset); operands: (method code, black, white, m_red, m_green, m_blue); lut: the 4096-byte table on src's device;
    dst: another flat uint8 buffer there (include/codetr_raw.h states the rule)"""
    _cabi.CALLS["raw"] += 1
    rc = load().codetr_raw_to_rgb_u8(_cabi.current_stream_ptr(src.device), src.data_ptr(), src.numel(), len(rows),
                                     (ctypes.c_int64 * (ROW_INTS * len(rows)))(*[int(v) for r in rows for v in r]),
                                     (ctypes.c_int64 * SETTING_INTS)(*[int(v) for v in operands]),
                                     lut.data_ptr(), dst.data_ptr(), dst.numel())
    _cabi.check(rc, "codetr_raw_to_rgb_u8")
