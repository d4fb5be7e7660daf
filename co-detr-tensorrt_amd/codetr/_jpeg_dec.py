"""ctypes binding of the JPEG decoder entry points of libcodetr_hip.so (C ABI: include/codetr_jpeg_dec.h, a companion
header of codetr_hip.h with a version of its own).  As in _jpeg.py the header is the one written copy: the signatures and
the CODETR_JPEGDEC_* constants are read from it with _cheader.parse, and a library that lacks an entry point is an
ImportError.  Flat integer and byte arrays only.
"""
import ctypes
import os

import numpy as np

from . import _cabi, _cheader

HEADER_PATH = os.path.join(os.path.dirname(_cheader.HEADER_PATH), "codetr_jpeg_dec.h")
if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the JPEG decoder binding is derived from it")
with open(HEADER_PATH) as _f:
    functions, defines = _cheader.parse(_f.read())

ABI_VERSION = defines["CODETR_JPEGDEC_ABI_VERSION"]
INFO_INTS = defines["CODETR_JPEGDEC_INFO_INTS"]
ROW_INTS = defines["CODETR_JPEGDEC_ROW_INTS"]
TABLE_BYTES = defines["CODETR_JPEGDEC_TABLE_BYTES"]
CHUNK_BYTES = defines["CODETR_JPEGDEC_CHUNK_BYTES"]   # raw scan bytes one lane owns
RUN_CHUNKS = defines["CODETR_JPEGDEC_RUN_CHUNKS"]     # chunks one workgroup settles among themselves
MAX_FILE_BYTES = defines["CODETR_JPEGDEC_MAX_FILE_BYTES"]
REASONS = {v: k[len("CODETR_JPEGDEC_R_"):].lower() for k, v in defines.items() if k.startswith("CODETR_JPEGDEC_R_")}
STATUS = {v: k[len("CODETR_JPEGDEC_S_"):].lower() for k, v in defines.items() if k.startswith("CODETR_JPEGDEC_S_")}

SIGNATURES = {name: (_cabi._CTYPE[_cheader.kind(ret, returned=True)], [_cabi._CTYPE[_cheader.kind(t)] for t, _ in params])
              for name, (ret, params) in functions.items()}

_cabi.CALLS.setdefault("jpeg_decode", 0)
_lib = None


def load():
    """the shared library with the decoder's prototypes set; ImportError when it is absent or older than this header"""
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
    ver = lib.codetr_jpegdec_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"{_cabi.LIB_PATH} has JPEG decoder ABI version {ver}, host expects {ABI_VERSION}; rebuild the "
                          "extension")
    _lib = lib
    return lib


def parse(data):
    """data: the file as a contiguous 1-D uint8 numpy array -> (return code, info int32 [INFO_INTS], tables uint8
    [TABLE_BYTES]); host only, no GPU.  The return code is 0 or a CODETR_E_*; info[6] holds the reason of E_UNSUPPORTED."""
    info = np.zeros(INFO_INTS, np.int32)
    tables = np.zeros(TABLE_BYTES, np.uint8)
    rc = load().codetr_jpegdec_parse(data.ctypes.data, data.size, info.ctypes.data, tables.ctypes.data)
    return rc, info, tables


def output_bytes(H, W) -> int:
    n = load().codetr_jpegdec_output_bytes(int(H), int(W))
    if n < 0:
        _cabi.check(n, "codetr_jpegdec_output_bytes")
    return n


def _rows(rows):
    return (ctypes.c_int64 * (ROW_INTS * len(rows)))(*[int(v) for row in rows for v in row])


def _infos(infos):
    return np.ascontiguousarray(np.asarray(infos, np.int32).reshape(-1, INFO_INTS))


def workspace_bytes(rows, infos) -> int:
    """bytes of workspace a decode of these rows (scan offset, scan bytes, H, W, dst offset) needs (host only)"""
    infos = _infos(infos)
    n = load().codetr_jpegdec_workspace_bytes(len(rows), _rows(rows), infos.ctypes.data)
    if n < 0:
        _cabi.check(n, "codetr_jpegdec_workspace_bytes")
    return n


def decode(scans, rows, infos, tables, dst, status, workspace):
    """scans: flat uint8 device buffer; rows: <= PREPROCESS_BATCH_MAX (scan offset, scan bytes, H, W, dst offset); infos:
    the parser's int32 [N, INFO_INTS] (host); tables: uint8 [N * TABLE_BYTES] on the device; dst: flat uint8 device buffer;
    status: int32 [N]; workspace: uint8 [>= workspace_bytes(...)], all on scans' device (include/codetr_jpeg_dec.h)"""
    _cabi.CALLS["jpeg_decode"] += 1
    infos = _infos(infos)
    rc = load().codetr_jpegdec_decode_u8(_cabi.current_stream_ptr(scans.device), scans.data_ptr(), scans.numel(), len(rows),
                                         _rows(rows), infos.ctypes.data, tables.data_ptr(), dst.data_ptr(), dst.numel(),
                                         status.data_ptr(), workspace.data_ptr(), workspace.numel())
    _cabi.check(rc, "codetr_jpegdec_decode_u8")
