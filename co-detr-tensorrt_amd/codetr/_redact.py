"""ctypes binding of the redaction entry points of libcodetr_hip.so (C ABI: include/codetr_redact.h, a companion header
of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures and
the CODETR_REDACT_* constants are read from it by _cabi.companion, and a library that lacks an entry point is an
ImportError.
"""
import ctypes

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_redact.h", "redact", "redaction")

ABI_VERSION = defines["CODETR_REDACT_ABI_VERSION"]
TILE = defines["CODETR_REDACT_TILE"]
MODES = {name: defines["CODETR_REDACT_" + name.upper()] for name in ("pixelate", "blur", "fill")}
SHAPES = {name: defines["CODETR_REDACT_" + name.upper()] for name in ("box", "ellipse")}
CELLS = (4, 8, 16, 32, 64)

_cabi.CALLS.setdefault("redact_detections", 0)


def _table(rows):
    return (ctypes.c_int64 * (3 * len(rows)))(*[int(v) for r in rows for v in r])


def work_bytes(rows, cell):
    """bytes of the "blur" workspace for the images `rows` [(offset, H, W)] (host only, no GPU)"""
    n = int(load().codetr_redact_work_bytes(len(rows), _table(rows), int(cell)))
    if n < 0:
        _cabi.check(n, "codetr_redact_work_bytes")
    return n


def redact_detections(buf, rows, boxes, scores, labels, count, select, mode, shape, cell, score_thr, expand, fill_rgb,
                      work):
    """buf: flat uint8 device buffer, redacted in place; rows: <= PREPROCESS_BATCH_MAX (offset, H, W); boxes [N, Q, 4] /
    scores [N, Q] in one dtype, labels [N, Q] int64, count [N] int32; select [C] uint8 on the device or None; mode / shape:
    the CODETR_REDACT_* codes; fill_rgb = 0xRRGGBB; work: uint8 of work_bytes(rows, cell) for "blur", else None
    (include/codetr_redact.h states the rule)"""
    _cabi.CALLS["redact_detections"] += 1
    N, Q = scores.shape
    name = "codetr_redact_detections_" + _cabi._SUFFIX[scores.dtype]
    rc = getattr(load(), name)(
        _cabi.current_stream_ptr(buf.device), buf.data_ptr(), buf.numel(), N, _table(rows), boxes.data_ptr(),
        scores.data_ptr(), labels.data_ptr(), count.data_ptr(), Q, _cabi._ptr(select),
        0 if select is None else select.numel(), int(mode), int(shape), int(cell), float(score_thr), float(expand),
        int(fill_rgb), _cabi._ptr(work), 0 if work is None else work.numel())
    _cabi.check(rc, name)
