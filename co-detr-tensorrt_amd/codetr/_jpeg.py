"""ctypes binding of the JPEG entry points of libcodetr_hip.so (C ABI: include/codetr_jpeg.h, the companion header of
codetr_hip.h with a version of its own).  As in _cabi.py the header is the one written copy: the signatures and the
CODETR_JPEG_* constants are read from it with _cheader.parse, and a library that lacks an entry point is an ImportError.
"""
import ctypes
import os

from . import _cabi, _cheader

HEADER_PATH = os.path.join(os.path.dirname(_cheader.HEADER_PATH), "codetr_jpeg.h")
if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the JPEG binding is derived from it")
with open(HEADER_PATH) as _f:
    functions, defines = _cheader.parse(_f.read())

ABI_VERSION = defines["CODETR_JPEG_ABI_VERSION"]
SUBSAMPLINGS = {"420": defines["CODETR_JPEG_420"], "444": defines["CODETR_JPEG_444"]}
HEADER_BYTES = defines["CODETR_JPEG_HEADER_BYTES"]
PASS_PIXELS = defines["CODETR_JPEG_PASS_PIXELS"]   # pixels of an MCU row one pass of a workgroup handles
BLOCK_BOUND = defines["CODETR_JPEG_BLOCK_BOUND"]   # the most scan bytes one 8x8 block can take

SIGNATURES = {name: (_cabi._CTYPE[_cheader.kind(ret, returned=True)], [_cabi._CTYPE[_cheader.kind(t)] for t, _ in params])
              for name, (ret, params) in functions.items()}

_cabi.CALLS.setdefault("jpeg_encode", 0)
_lib = None


def load():
    """the shared library with the JPEG prototypes set; ImportError when it is absent or older than this header"""
    global _lib
    if _lib is not None:
        return _lib
    _cabi.load()
    lib = _cabi._lib   # (the plain library: the JPEG entries are not part of a launch plan and are never recorded)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{_cabi.LIB_PATH} does not export {name}; rebuild the extension") from e
        fn.restype = res
        fn.argtypes = args
    ver = lib.codetr_jpeg_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"{_cabi.LIB_PATH} has JPEG ABI version {ver}, host expects {ABI_VERSION}; rebuild the extension")
    _lib = lib
    return lib


def _table(rows):
    return (ctypes.c_int64 * (3 * len(rows)))(*[int(v) for row in rows for v in row])


def header(H, W, quality, subsampling) -> bytes:
    """SOI up to and including SOS of an H x W file (host only, no GPU); subsampling: a value of SUBSAMPLINGS"""
    out = (ctypes.c_ubyte * HEADER_BYTES)()
    n = load().codetr_jpeg_header(int(H), int(W), int(quality), int(subsampling), out, HEADER_BYTES)
    if n < 0:
        _cabi.check(n, "codetr_jpeg_header")
    return bytes(out[:n])


def scan_bound(H, W, subsampling) -> int:
    """a proven upper bound of the scan bytes of an H x W image (host only)"""
    n = load().codetr_jpeg_scan_bound(int(H), int(W), int(subsampling))
    if n < 0:
        _cabi.check(n, "codetr_jpeg_scan_bound")
    return n


def workspace_bytes(rows, subsampling, out_stride) -> int:
    """bytes of workspace an encode of these (offset, H, W) rows needs (host only)"""
    n = load().codetr_jpeg_workspace_bytes(len(rows), _table(rows), int(subsampling), int(out_stride))
    if n < 0:
        _cabi.check(n, "codetr_jpeg_workspace_bytes")
    return n


def encode(buf, rows, quality, subsampling, out, out_stride, lengths, workspace):
    """buf: flat uint8 device buffer; rows: <= PREPROCESS_BATCH_MAX (offset, H, W); out: uint8 [>= N * out_stride],
    lengths: int32 [N], workspace: uint8 [>= workspace_bytes(...)], all on buf's device (include/codetr_jpeg.h)"""
    _cabi.CALLS["jpeg_encode"] += 1
    rc = load().codetr_jpeg_encode_u8(_cabi.current_stream_ptr(buf.device), buf.data_ptr(), buf.numel(), len(rows),
                                      _table(rows), int(quality), int(subsampling), out.data_ptr(), int(out_stride),
                                      lengths.data_ptr(), workspace.data_ptr(), workspace.numel())
    _cabi.check(rc, "codetr_jpeg_encode_u8")
