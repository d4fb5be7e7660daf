"""ctypes binding of the contrast-enhancement entry points of libcodetr_hip.so (C ABI: include/codetr_enhance.h, a companion
header of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures and the
CODETR_ENHANCE_* constants are read from it by _cabi.companion, and a library that lacks an entry point is an
ImportError.
"""
import ctypes

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_enhance.h", "enhance", "enhancement")

ABI_VERSION = defines["CODETR_ENHANCE_ABI_VERSION"]
ROW_INTS = defines["CODETR_ENHANCE_ROW_INTS"]
MAX_GRID = defines["CODETR_ENHANCE_MAX_GRID"]
MAX_TILE = defines["CODETR_ENHANCE_MAX_TILE"]
SLICE_PIXELS = defines["CODETR_ENHANCE_SLICE_PIXELS"]
MAX_SLICES = defines["CODETR_ENHANCE_MAX_SLICES"]
BOUND_HALVES = defines["CODETR_ENHANCE_BOUND_HALVES"]

_cabi.CALLS.setdefault("enhance", 0)


def _table(rows):
    return (ctypes.c_int64 * (ROW_INTS * len(rows)))(*[int(v) for r in rows for v in r])


def workspace_bytes(rows):
    """the scratch bytes one call on these rows needs; the entry point's own checks of the sizes and grids apply"""
    n = load().codetr_enhance_workspace_bytes(len(rows), _table(rows))
    if n < 0:
        _cabi.check(n, "codetr_enhance_workspace_bytes")
    return n


def enhance(src, rows, dst, ws):
    """src: flat uint8 device buffer; rows: <= PREPROCESS_BATCH_MAX (H, W, src offset, src pitch, dst offset, dst pitch, gy,
    gx, C); dst: another flat uint8 buffer on src's device, or src itself with every destination its source (in place); ws:
    a device tensor of at least workspace_bytes(rows) bytes (include/codetr_enhance.h states the rule)"""
    _cabi.CALLS["enhance"] += 1
    rc = load().codetr_enhance_rgb_u8(_cabi.current_stream_ptr(src.device), src.data_ptr(), src.numel(), len(rows), _table(rows),
                                      dst.data_ptr(), dst.numel(), ws.data_ptr(), ws.numel() * ws.element_size())
    _cabi.check(rc, "codetr_enhance_rgb_u8")
