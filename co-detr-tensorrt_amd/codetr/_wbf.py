"""ctypes binding of the weighted-boxes-fusion entry points of libcodetr_hip.so (C ABI: include/codetr_wbf.h, a companion
header of codetr_hip.h with a version of its own).  As in _assign.py the header is the one written copy: the signatures
and the CODETR_WBF_* constants are read from it with _cheader.parse, and a library that lacks an entry point is an
ImportError.
"""
import ctypes
import os

from . import _cabi, _cheader

HEADER_PATH = os.path.join(os.path.dirname(_cheader.HEADER_PATH), "codetr_wbf.h")
if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the WBF binding is derived from it")
with open(HEADER_PATH) as _f:
    functions, defines = _cheader.parse(_f.read())

ABI_VERSION = defines["CODETR_WBF_ABI_VERSION"]
MAX_CANDIDATES = defines["CODETR_WBF_MAX_CANDIDATES"]
CONF_TYPES = {"avg": defines["CODETR_WBF_CONF_AVG"], "max": defines["CODETR_WBF_CONF_MAX"]}

SIGNATURES = {name: (_cabi._CTYPE[_cheader.kind(ret, returned=True)], [_cabi._CTYPE[_cheader.kind(t)] for t, _ in params])
              for name, (ret, params) in functions.items()}

_cabi.CALLS.setdefault("wbf_merge", 0)
_lib = None


def load():
    """the shared library with the WBF prototypes set; ImportError when it is absent or older than this header"""
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
    ver = lib.codetr_wbf_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"{_cabi.LIB_PATH} has WBF ABI version {ver}, host expects {ABI_VERSION}; rebuild the extension")
    _lib = lib
    return lib


def wbf_merge(boxes, scores, labels, count, flip_mask, width, weights, conf_type, iou_threshold, skip_box_thr, max_keep,
              boxes_out, scores_out, labels_out, index_out, count_out, votes_out):
    """boxes [V,N,Q,4] / scores [V,N,Q] in one dtype, labels [V,N,Q] int64, count [V,N] int32, width [N] fp32; weights
    None or V floats; conf_type a value of CONF_TYPES; outputs [N,K,..] with K = max_keep, or V*Q when max_keep <= 0
    (include/codetr_wbf.h)"""
    _cabi.CALLS["wbf_merge"] += 1
    V, N, Q = scores.shape
    name = "codetr_wbf_merge_" + _cabi._SUFFIX[scores.dtype]
    w = None if weights is None else (ctypes.c_float * V)(*[float(v) for v in weights])
    rc = getattr(load(), name)(
        _cabi.current_stream_ptr(scores.device), boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr(),
        V, N, Q, int(flip_mask), width.data_ptr(), w, int(conf_type), float(iou_threshold), float(skip_box_thr),
        int(max_keep), boxes_out.data_ptr(), scores_out.data_ptr(), labels_out.data_ptr(), index_out.data_ptr(),
        count_out.data_ptr(), votes_out.data_ptr())
    _cabi.check(rc, name)
