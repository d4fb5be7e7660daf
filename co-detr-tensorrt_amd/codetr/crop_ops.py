"""The Inferencer's object crops (hip_ops re-exports these names): the regions under a chunk's detections resampled, with
antialiasing, to one fixed size for a second-stage model -- uint8 HWC crops and, when asked, the normalised CHW tensors.
GPU-only, as hip_ops; include/codetr_crops.h states the rule, csrc/crops.hip holds the kernels.
"""
import torch

from . import _cabi, _crops
from . import _operands as _check

__all__ = ["CROPS", "CROP_FITS", "crop_settings", "crop_detections"]

# `size` (w, h) has no default: a second-stage model fixes it.  tensor: None, or dict(mean, std, dtype) for the
# normalised form; download: False keeps the uint8 crops on the device (the Inferencer reads it)
CROPS = dict(size=None, score_thr=0.3, expand=0.0, fit="stretch", pad_value=(114, 114, 114), max_per_img=32, tensor=None,
             download=True)
CROP_FITS = tuple(_crops.FITS)
_TENSOR = dict(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=torch.float16)


def _size(v):
    side = _check.whole(_crops.MIN_SIDE, _crops.MAX_SIDE)
    if not isinstance(v, (tuple, list)) or len(v) != 2:
        raise _check._Not(f"(w, h), each an integer in {_crops.MIN_SIDE}..{_crops.MAX_SIDE}")
    try:
        return (side(v[0]), side(v[1]))
    except _check._Not:
        raise _check._Not(f"(w, h), each an integer in {_crops.MIN_SIDE}..{_crops.MAX_SIDE}") from None


def _triple(nonzero):
    def check(v):
        what = "three finite numbers" + (", none zero" if nonzero else "")
        if not isinstance(v, (tuple, list)) or len(v) != 3:
            raise _check._Not(what)
        out = tuple(_check.number()(c) for c in v)
        if nonzero and any(c == 0 for c in out):
            raise _check._Not(what)
        return out
    return check


def _dtype(v):
    if not isinstance(v, torch.dtype) or v not in _crops.TENSOR_TYPES:
        raise _check._Not("torch.float32, torch.float16 or torch.bfloat16")
    return v


def _tensor(v):
    if v is None:
        return None
    if not isinstance(v, dict):
        raise _check._Not("None or a dict with keys of ['dtype', 'mean', 'std']")
    try:
        return _check.validated("tensor", _TENSOR, v, dict(mean=_triple(False), std=_triple(True), dtype=_dtype), sep=": ")
    except ValueError as e:
        raise ValueError(f"crops: {e}") from None


def crop_settings(settings=None):
    """the settings of crop_detections, validated and completed from CROPS -> a new dict.  ValueError, naming the key, for
    an unknown key, a missing or out-of-range size, a fit outside CROP_FITS, an expand outside [0, 1], a score_thr that is
    not a number, a pad_value that is not three whole values in 0..255, a max_per_img outside 1..256, a tensor that is not
    None or dict(mean, std, dtype), a download that is False without a tensor."""
    st = _check.validated("crops", CROPS, settings, dict(
        size=_size, fit=_check.one_of(CROP_FITS), score_thr=_check.number(finite=False), expand=_check.number(0, 1),
        pad_value=_check.colour, max_per_img=_check.whole(1, _crops.MAX_PER_IMG), tensor=_tensor), sep=": ")
    if not isinstance(st["download"], bool):
        raise ValueError(f"crops: download must be a bool, got {st['download']!r}")
    if not st["download"] and st["tensor"] is None:
        raise ValueError("crops: download=False leaves nothing to return without a tensor")
    return st


def crop_detections(buf_u8, rows, dets, settings=None, select=None):
    """Crops of the detected objects in two launches per PREPROCESS_BATCH_MAX images and without a synchronisation
    (csrc/crops.hip; include/codetr_crops.h states the rule): per image the first settings['max_per_img'] detections, in
    row order, with a score of at least settings['score_thr'], a selected label and a non-empty region -- the box grown
    by settings['expand'] and clipped to the image -- are resampled with the antialiased triangle filter to
    settings['size'] = (w, h); fit "pad" keeps the aspect ratio and fills with settings['pad_value'].
      buf_u8    one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's); only read
      rows      (offset, H, W) per image
      dets      Detections / SoftDetections over [N, Q] rows, N = len(rows), Q <= 4096, boxes in image coordinates
      settings  the keys of CROPS; size is required
      select    [C] uint8 on the device, 1 = crop this label; None = every label
    -> (crops [N, M, h, w, 3] uint8, counts [N] int32) and, with settings['tensor'], the normalised [N, M, 3, h, w] in its
    dtype; M = max_per_img, and the slots beyond an image's count are left unwritten.  ValueError for Q > 4096, a bad
    setting, a wrong dtype or shape, CPU tensors.  Nothing is launched when N == 0 or Q == 0 (the counts are zeros)."""
    st = crop_settings(settings)
    rows = _check.image_rows("crop_detections", buf_u8, rows, _cabi.DRAW_MAX_SIDE)
    if select is not None:
        _check.same_gpu("crop_detections", buf_u8.device, select=select)
        if select.dtype != torch.uint8 or select.dim() != 1 or select.numel() == 0:
            raise ValueError("crop_detections: select must be a [C] uint8 table, C > 0")
    N, Q = _check.detections("crop_detections", dets, buf_u8.device, _cabi.DRAW_MAX_Q, len(rows))
    (w, h), M, dev = st["size"], st["max_per_img"], buf_u8.device
    crops = torch.empty((N, M, h, w, 3), dtype=torch.uint8, device=dev)
    tensor = None if st["tensor"] is None else torch.empty((N, M, 3, h, w), dtype=st["tensor"]["dtype"], device=dev)
    if N == 0 or Q == 0:
        counts = torch.zeros((N,), dtype=torch.int32, device=dev)
        return (crops, counts) if tensor is None else (crops, counts, tensor)
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    table = torch.empty((N, M, _crops.TABLE_INTS), dtype=torch.int32, device=dev)
    boxes, scores, labels, count = (t.contiguous() for t in (dets.boxes, dets.scores, dets.labels, dets.count))
    select = None if select is None else select.contiguous()
    pad = st["pad_value"]
    mean, std = (None, None) if tensor is None else (st["tensor"]["mean"], st["tensor"]["std"])
    with torch.cuda.device(dev):
        for i, j in _check.chunks(N):
            _crops.crop_detections(buf_u8, rows[i:j], boxes[i:j], scores[i:j], labels[i:j], count[i:j], select, (w, h), M,
                                   _crops.FITS[st["fit"]], st["score_thr"], st["expand"], (pad[0] << 16) | (pad[1] << 8) | pad[2],
                                   crops[i:j], counts[i:j], table[i:j], None if tensor is None else tensor[i:j], mean, std)
    return (crops, counts) if tensor is None else (crops, counts, tensor)
