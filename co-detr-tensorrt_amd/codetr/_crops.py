"""ctypes binding of the object-crop entry points of libcodetr_hip.so (C ABI: include/codetr_crops.h, a companion header
of codetr_hip.h with a version of its own).  The header is the one written copy: the signatures and the CODETR_CROPS_*
constants are read from it by _cabi.companion, and a library that lacks an entry point is an ImportError.
"""
import ctypes

import torch

from . import _cabi

HEADER_PATH, functions, defines, SIGNATURES, load = _cabi.companion("codetr_crops.h", "crops", "crops")

ABI_VERSION = defines["CODETR_CROPS_ABI_VERSION"]
FITS = {name: defines["CODETR_CROPS_" + name.upper()] for name in ("stretch", "pad")}
MIN_SIDE, MAX_SIDE = defines["CODETR_CROPS_MIN_SIDE"], defines["CODETR_CROPS_MAX_SIDE"]
MAX_PER_IMG = defines["CODETR_CROPS_MAX_PER_IMG"]
TABLE_INTS = defines["CODETR_CROPS_TABLE_INTS"]
TENSOR_TYPES = {torch.float32: defines["CODETR_CROPS_TENSOR_F32"], torch.float16: defines["CODETR_CROPS_TENSOR_F16"],
                torch.bfloat16: defines["CODETR_CROPS_TENSOR_BF16"]}

_cabi.CALLS.setdefault("crop_detections", 0)


def crop_detections(buf, rows, boxes, scores, labels, count, select, size, max_per_img, fit, score_thr, expand, pad_rgb,
                    crops, counts, table, tensor=None, mean=None, std=None):
    """buf: flat uint8 device buffer, read only; rows: <= PREPROCESS_BATCH_MAX (offset, H, W); boxes [N, Q, 4] / scores
    [N, Q] in one dtype, labels [N, Q] int64, count [N] int32; select [C] uint8 on the device or None; size = (w, h); fit:
    the CODETR_CROPS_* code; pad_rgb = 0xRRGGBB; crops [N, M, h, w, 3] uint8, counts [N] int32 and table [N, M, TABLE_INTS]
    int32 are written; tensor [N, M, 3, h, w] f32 / f16 / bf16 with mean and std, or None (include/codetr_crops.h states
    the rule)"""
    _cabi.CALLS["crop_detections"] += 1
    N, Q = scores.shape
    f3 = ctypes.c_float * 3
    name = "codetr_crop_detections_" + _cabi._SUFFIX[scores.dtype]
    rc = getattr(load(), name)(
        _cabi.current_stream_ptr(buf.device), buf.data_ptr(), buf.numel(), N,
        (ctypes.c_int64 * (3 * len(rows)))(*[int(v) for r in rows for v in r]), boxes.data_ptr(), scores.data_ptr(),
        labels.data_ptr(), count.data_ptr(), Q, _cabi._ptr(select), 0 if select is None else select.numel(), int(size[0]),
        int(size[1]), int(max_per_img), int(fit), float(score_thr), float(expand), int(pad_rgb), crops.data_ptr(),
        counts.data_ptr(), table.data_ptr(), _cabi._ptr(tensor), 0 if tensor is None else TENSOR_TYPES[tensor.dtype],
        None if tensor is None else f3(*[float(v) for v in mean]), None if tensor is None else f3(*[float(v) for v in std]))
    _cabi.check(rc, name)
