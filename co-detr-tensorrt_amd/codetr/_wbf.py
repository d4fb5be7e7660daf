"""ctypes binding of the weighted-boxes-fusion entry points of libcodetr_hip.so (C ABI: include/codetr_wbf.h, a companion
header of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures
and the CODETR_WBF_* constants are read from it by _cabi.companion, and a library that lacks an entry point is an
ImportError.
"""
import ctypes

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_wbf.h", "wbf", "WBF")

ABI_VERSION = defines["CODETR_WBF_ABI_VERSION"]
MAX_CANDIDATES = defines["CODETR_WBF_MAX_CANDIDATES"]
CONF_TYPES = {"avg": defines["CODETR_WBF_CONF_AVG"], "max": defines["CODETR_WBF_CONF_MAX"]}

_cabi.CALLS.setdefault("wbf_merge", 0)


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
