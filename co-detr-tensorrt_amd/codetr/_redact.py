"""ctypes binding of the redaction entry points of libcodetr_hip.so (C ABI: include/codetr_redact.h, a companion header
of codetr_hip.h with a version of its own).  As in _appearance.py the header is the one written copy: the signatures and
the CODETR_REDACT_* constants are read from it with _cheader.parse, and a library that lacks an entry point is an
ImportError.
"""
import ctypes
import os

from . import _cabi, _cheader

HEADER_PATH = os.path.join(os.path.dirname(_cheader.HEADER_PATH), "codetr_redact.h")
if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the redaction binding is derived from it")
with open(HEADER_PATH) as _f:
    functions, defines = _cheader.parse(_f.read())

ABI_VERSION = defines["CODETR_REDACT_ABI_VERSION"]
TILE = defines["CODETR_REDACT_TILE"]
MODES = {name: defines["CODETR_REDACT_" + name.upper()] for name in ("pixelate", "blur", "fill")}
SHAPES = {name: defines["CODETR_REDACT_" + name.upper()] for name in ("box", "ellipse")}
CELLS = (4, 8, 16, 32, 64)

SIGNATURES = {name: (_cabi._CTYPE[_cheader.kind(ret, returned=True)], [_cabi._CTYPE[_cheader.kind(t)] for t, _ in params])
              for name, (ret, params) in functions.items()}

_cabi.CALLS.setdefault("redact_detections", 0)
_lib = None


def load():
    """the shared library with the redaction prototypes set; ImportError when it is absent or older than this header"""
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
    ver = lib.codetr_redact_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"{_cabi.LIB_PATH} has redaction ABI version {ver}, host expects {ABI_VERSION}; rebuild the "
                          "extension")
    _lib = lib
    return lib


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
