"""The Inferencer's operators on detections (hip_ops re-exports them): NMS and soft-NMS post-processing into the packed
result, and the merges of several views' results -- test-time augmentation, weighted boxes fusion, sliced inference.
GPU-only, as hip_ops.
"""
import collections
import math

import torch

from . import _cabi, _wbf
from . import _operands as _check
from ._operands import _gpu

# the public names (hip_ops re-exports exactly these)
__all__ = [
    "batched_nms", "Detections", "SoftDetections", "postprocess_detections", "detections_to_host",
    "postprocess_detections_soft", "soft_nms", "TTA_MAX_VIEWS", "TTA_MAX_CANDIDATES", "tta_merge", "WbfDetections",
    "WBF_MAX_CANDIDATES", "WBF", "wbf_settings", "wbf_merge", "weighted_boxes_fusion", "SLICE_MAX_VIEWS",
    "SLICE_MERGE", "slice_merge_settings", "slice_merge",
]


def batched_nms(boxes, scores, labels, iou_threshold):
    """torchvision.ops.batched_nms semantics (per-class greedy hard NMS): indices of the kept boxes in descending
    score order.  IoU arithmetic in fp32 on the given boxes."""
    _gpu(boxes, "batched_nms")
    if boxes.shape[0] == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores.float(), descending=True, stable=True)[1]
    with torch.cuda.device(boxes.device):
        keep = _cabi.batched_nms_sorted(boxes.float()[order].contiguous(), labels.to(torch.int64)[order].contiguous(),
                                        iou_threshold)
    return order[keep]


# postprocess_detections' result: boxes [N,Q,4] / scores [N,Q] (input dtype), labels [N,Q] int64, count [N] int32 --
# image i's detections are rows [:count[i]] -- all four views of the one byte buffer `packed`
Detections = collections.namedtuple("Detections", "boxes scores labels count packed")
# postprocess_detections_soft's and tta_merge's result: the fields of Detections + index [N,Q] int32, the input index
# of every output row -- five views of the one byte buffer `packed`
SoftDetections = collections.namedtuple("SoftDetections", "boxes scores labels count index packed")


def packed_detections(N, Q, dtype, index=False, votes=False, packed=None, device=None, zeros=False):
    """The packed result over [N, Q] rows, and the one statement of its layout: labels int64 [N,Q], count int32 [N],
    [index int32 [N,Q],] [votes int32 [N,Q],] boxes [N,Q,4], scores [N,Q] (`dtype`), back to back in this order.
    `packed`: the byte buffer to view; None: a new one on `device` for a launch to fill -- `zeros`: nothing will be
    launched, every count is 0.  -> Detections, SoftDetections (index) or WbfDetections (index and votes)."""
    es = dtype.itemsize
    o1 = N * Q * 8
    o2 = o1 + N * 4
    o3 = o2 + (N * Q * 4 if index else 0)
    o4 = o3 + (N * Q * 4 if votes else 0)
    o5 = o4 + N * Q * 4 * es
    o6 = o5 + N * Q * es
    if packed is None:
        packed = (torch.zeros if zeros else torch.empty)((o6,), dtype=torch.uint8, device=device)
    boxes, scores = packed[o4:o5].view(dtype).view(N, Q, 4), packed[o5:o6].view(dtype).view(N, Q)
    labels, count = packed[:o1].view(torch.int64).view(N, Q), packed[o1:o2].view(torch.int32)
    if not index:
        return Detections(boxes, scores, labels, count, packed)
    rows = packed[o2:o3].view(torch.int32).view(N, Q)
    if not votes:
        return SoftDetections(boxes, scores, labels, count, rows, packed)
    return WbfDetections(boxes, scores, labels, count, rows, packed[o3:o4].view(torch.int32).view(N, Q), packed)


def _post_operands(name, boxes, scores, labels, divisors):
    """the operand checks of postprocess_detections and postprocess_detections_soft (`name`) -> N, Q"""
    dtype = scores.dtype
    if dtype not in _check.FLOATS or boxes.dtype != dtype or divisors.dtype != dtype:
        raise ValueError(f"{name}: boxes, scores and divisors in one dtype of f16 / bf16 / f32")
    shapes = f"{name}: boxes [N,Q,4], scores [N,Q], labels [N,Q], divisors [N,4]"
    if scores.dim() != 2:
        raise ValueError(shapes)
    N, Q = scores.shape
    if tuple(boxes.shape) != (N, Q, 4) or tuple(labels.shape) != (N, Q) or tuple(divisors.shape) != (N, 4):
        raise ValueError(shapes)
    return N, Q


def postprocess_detections(boxes, scores, labels, divisors, score_threshold=None, iou_threshold=None):
    """Inferencer.postprocess_predictions + run_inference's `boxes / scale_factor` for a whole batch in one launch
    (csrc/prepost.hip): boxes [N,Q,4], scores [N,Q], divisors [N,4] in one of f16 / bf16 / f32, labels [N,Q] int64,
    Q <= 1024.  score_threshold: keep `scores > score_threshold` (compared in the scores' dtype; None: no threshold);
    iou_threshold: per-class NMS in descending score order (None: none, index order kept).  -> Detections, compacted
    per image; `detections_to_host` fetches all of it in one copy."""
    _gpu(scores, "postprocess_detections")
    N, Q = _post_operands("postprocess_detections", boxes, scores, labels, divisors)
    nothing = N == 0 or Q == 0
    out = packed_detections(N, Q, scores.dtype, device=scores.device, zeros=nothing)
    if nothing:
        return out
    with torch.cuda.device(scores.device):
        _cabi.postprocess_detections(boxes.contiguous(), scores.contiguous(), labels.to(torch.int64).contiguous(),
                                     divisors.contiguous(), score_threshold, iou_threshold, out.boxes, out.scores,
                                     out.labels, out.count)
    return out


def detections_to_host(dets):
    """postprocess_detections' (or postprocess_detections_soft's, `index` included) result on the host: one
    device-to-host copy of the packed buffer"""
    N, Q = dets.scores.shape
    wbf = isinstance(dets, WbfDetections)
    return packed_detections(N, Q, dets.scores.dtype, wbf or isinstance(dets, SoftDetections), wbf, dets.packed.cpu())


def _soft_method(method):
    if method == "gaussian":
        raise NotImplementedError("soft-NMS method 'gaussian' is not provided (exp() cannot be held bit-exact against "
                                  "the CPU reference and no shipped config uses it): 'linear' or 'naive'")
    if method not in _cabi.SOFTNMS_METHODS:
        raise ValueError(f"soft-NMS method must be 'linear' or 'naive', got {method!r}")
    return _cabi.SOFTNMS_METHODS[method]


def postprocess_detections_soft(boxes, scores, labels, divisors, score_threshold=None, iou_threshold=0.3,
                                method="linear", min_score=1e-3, max_per_img=None):
    """The post-processing the model configs specify (test_cfg[0]: nms type 'soft_nms', max_per_img) + run_inference's
    `boxes / scale_factor` for a whole batch in one launch (csrc/prepost.hip; semantics: include/codetr_hip.h): mmcv's
    soft-NMS per class -- overlapping boxes are not removed but their scores decayed by 1 - IoU (`linear`) or set to 0
    (`naive`) when IoU >= iou_threshold, a box leaves once its score is < min_score --, the detections sorted by decayed
    score, the first max_per_img kept (None: all).  Operands as postprocess_detections; the defaults are mmcv's.
    -> SoftDetections: scores are the decayed ones, `index` the query index of every row."""
    _gpu(scores, "postprocess_detections_soft")
    m = _soft_method(method)
    N, Q = _post_operands("postprocess_detections_soft", boxes, scores, labels, divisors)
    nothing = N == 0 or Q == 0
    out = packed_detections(N, Q, scores.dtype, index=True, device=scores.device, zeros=nothing)
    if nothing:
        return out
    with torch.cuda.device(scores.device):
        _cabi.postprocess_softnms(boxes.contiguous(), scores.contiguous(), labels.to(torch.int64).contiguous(),
                                  divisors.contiguous(), score_threshold, m, iou_threshold, min_score,
                                  0 if max_per_img is None else int(max_per_img), out.boxes, out.scores, out.labels,
                                  out.index, out.count)
    return out


def soft_nms(boxes, scores, labels, iou_threshold, method="linear", min_score=1e-3):
    """mmcv batched_nms(..., nms_cfg=dict(type='soft_nms')) semantics for one image's detections (boxes [n,4],
    scores [n], labels [n]; n <= 1024), the counterpart of `batched_nms`: -> (new_scores, keep), the decayed scores of
    the kept boxes in descending order (dtype of `scores`) and their indices.  The N = 1 launch of
    postprocess_detections_soft with unit divisors."""
    _gpu(boxes, "soft_nms")
    _soft_method(method)
    n = boxes.shape[0]
    if n == 0:
        return scores.new_empty((0,)), torch.empty((0,), dtype=torch.int64, device=boxes.device)
    if n > _cabi.POSTPROCESS_MAX_Q:
        raise ValueError(f"soft_nms: at most {_cabi.POSTPROCESS_MAX_Q} boxes per call, got {n}")
    dtype = scores.dtype if scores.dtype in _check.FLOATS else torch.float32
    dets = postprocess_detections_soft(boxes.to(dtype)[None], scores.to(dtype)[None], labels[None],
                                       torch.ones((1, 4), dtype=dtype, device=boxes.device), None, iou_threshold, method,
                                       min_score, None)
    c = int(dets.count[0])
    return dets.scores[0, :c].to(scores.dtype), dets.index[0, :c].to(torch.int64)


TTA_MAX_VIEWS = _cabi.TTA_MAX_VIEWS
TTA_MAX_CANDIDATES = _cabi.TTA_MAX_CANDIDATES


def _tta_mode(nms):
    """tta_cfg.nms -> (mode of codetr_tta_merge_*, iou_threshold, min_score); mmcv's defaults where a key is absent"""
    kind = nms.get("type", "nms")
    if kind == "nms":
        return _cabi.TTA_NMS_MODES["nms"], float(nms.get("iou_threshold", 0.5)), 0.0
    if kind != "soft_nms":
        raise NotImplementedError(f"tta nms type {kind!r}: 'nms' and 'soft_nms' are built")
    method = nms.get("method", "linear")
    _soft_method(method)   # 'gaussian' raises NotImplementedError, an unknown name ValueError
    return _cabi.TTA_NMS_MODES[method], float(nms.get("iou_threshold", 0.3)), float(nms.get("min_score", 1e-3))


def _entries(name, dets, what="detections"):
    """one result of postprocess_detections / _soft, or a list of them -> (the list, dtype, device, Q); ValueError unless
    every entry is [rows, Q] in one dtype of f16 / bf16 / f32"""
    dets = list(dets) if isinstance(dets, (list, tuple)) and not hasattr(dets, "scores") else [dets]
    if not dets:
        raise ValueError(f"{name}: no {what}")
    scores0 = dets[0].scores
    _gpu(scores0, name)
    dtype, Q = scores0.dtype, scores0.shape[-1]
    if dtype not in _check.FLOATS:
        raise ValueError(f"{name}: detections in f16, bf16 or f32")
    if any(d.scores.dim() != 2 or d.scores.shape[1] != Q or d.scores.dtype != dtype for d in dets):
        raise ValueError(f"{name}: every entry [rows, Q] detections of one dtype")
    return dets, dtype, scores0.device, Q


def _cat(dets):
    """the entries concatenated in order -> contiguous boxes, scores, labels, count"""
    one = len(dets) == 1
    return ((getattr(dets[0], f) if one else torch.cat([getattr(d, f) for d in dets])).contiguous()
            for f in ("boxes", "scores", "labels", "count"))


def _merge_operands(name, view_dets, flips, widths):
    """the operand checks of tta_merge and wbf_merge (`name`) -> (dtype, device, N, V, Q, boxes, scores, labels, count,
    flips, widths): the entries concatenated in order, `widths` a tensor"""
    view_dets, dtype, dev, Q = _entries(name, view_dets, "views")
    if not torch.is_tensor(widths):
        widths = torch.tensor([float(w) for w in widths], dtype=torch.float32)
    N = widths.numel()
    if N == 0 or any(d.scores.shape[0] % N for d in view_dets):
        raise ValueError(f"{name}: every entry [views * N, Q] detections of one dtype, N = len(widths) > 0")
    V = sum(d.scores.shape[0] for d in view_dets) // N
    flips = [bool(f) for f in flips]
    if len(flips) != V:
        raise ValueError(f"{name}: {V} views but {len(flips)} flip flags")
    if V > TTA_MAX_VIEWS or V * Q > TTA_MAX_CANDIDATES:
        raise ValueError(f"{name}: at most {TTA_MAX_VIEWS} views and {TTA_MAX_CANDIDATES} candidates per image, "
                         f"got {V} views of {Q}")
    return (dtype, dev, N, V, Q, *_cat(view_dets), flips, widths)


def _merged_result(N, V, Q, dtype, dev, max_per_img, nothing, votes=False):
    """-> (keep, the packed result of a merge over [N, K] rows, K = max_per_img or V * Q); `nothing`: zero-filled, the
    caller returns it without a launch"""
    keep = 0 if max_per_img is None else int(max_per_img)
    return keep, packed_detections(N, keep if keep > 0 else V * Q, dtype, True, votes, device=dev, zeros=nothing)


def tta_merge(view_dets, flips, widths, nms=None, max_per_img=None):
    """mmdet DetTTAModel._merge_single_sample for a batch of N images in one launch (csrc/prepost.hip; semantics:
    include/codetr_hip.h): the views' detections un-flipped, concatenated, batched_nms(nms), the best max_per_img kept.
      view_dets    the per-view results of postprocess_detections / postprocess_detections_soft, boxes already in
                   original-image coordinates.  Each entry holds one or more views of all N images, view-major (its
                   leading dimension is a multiple of N); the entries are concatenated in order, so view v is row block v
      flips        one bool per view: the view was flipped horizontally
      widths       [N] original image widths (a tensor on the device, or numbers)
      nms          dict(type='nms' | 'soft_nms', iou_threshold, [method 'linear' | 'naive', min_score]); None: hard, 0.5
      max_per_img  None: all
    -> SoftDetections over [N, K] rows (K = max_per_img, or V * Q): `index` is c = v * Q + j of every row, scores are
    the decayed ones in the soft modes; `detections_to_host` fetches all of it in one copy."""
    mode, iou, min_score = _tta_mode(dict(nms) if nms is not None else {})
    dtype, dev, N, V, Q, boxes, scores, labels, count, flips, widths = _merge_operands("tta_merge", view_dets, flips, widths)
    keep, out = _merged_result(N, V, Q, dtype, dev, max_per_img, Q == 0)
    if Q == 0:
        return out
    with torch.cuda.device(dev):
        _cabi.tta_merge(boxes.view(V, N, Q, 4), scores.view(V, N, Q), labels.view(V, N, Q), count.view(V, N),
                        sum(1 << v for v, f in enumerate(flips) if f), widths.to(dev, torch.float32).contiguous(), mode,
                        iou, min_score, keep, out.boxes, out.scores, out.labels, out.index, out.count)
    return out


# wbf_merge's result: the fields of SoftDetections + votes [N,K] int32, the number of candidates fused into every row --
# six views of the one byte buffer `packed` (labels, count, index, votes, boxes, scores in this order)
WbfDetections = collections.namedtuple("WbfDetections", "boxes scores labels count index votes packed")
WBF_MAX_CANDIDATES = _wbf.MAX_CANDIDATES
WBF = dict(iou_threshold=0.55, skip_box_thr=0.0, conf_type="avg", weights=None)   # ensemble_boxes' defaults


def wbf_settings(d=None):
    """the `wbf` dict of a weighted boxes fusion, validated and completed from WBF -> dict(iou_threshold, skip_box_thr,
    conf_type 'avg' | 'max', weights None or a list of positive floats)"""
    if d is not None and not isinstance(d, dict):
        raise ValueError(f"wbf must be None or a dict with keys of {sorted(WBF)}")
    def conf_type(v):
        if v in ("box_and_model_avg", "absent_model_aware_avg"):
            raise NotImplementedError(f"wbf conf_type {v!r} is not built: 'avg' or 'max'")
        return _check.one_of(_wbf.CONF_TYPES)(v)

    out = _check.validated("wbf", WBF, d, dict(conf_type=conf_type, iou_threshold=_check.number(coerce=True),
                                               skip_box_thr=_check.number(coerce=True)))
    if out["weights"] is not None:
        out["weights"] = [float(w) for w in out["weights"]]
        if not out["weights"] or any(not math.isfinite(w) or w <= 0 for w in out["weights"]):
            raise ValueError("wbf weights: None or a non-empty list of finite positive numbers")
    return out


def wbf_merge(view_dets, flips, widths, wbf=None, max_per_img=None):
    """Weighted boxes fusion of the views' detections for a batch of N images in one launch (csrc/prepost.hip; the rule:
    include/codetr_wbf.h): un-flipped, clustered per label in descending confidence, every cluster emitted as its
    confidence-weighted mean box with a score that says how many views agreed; the best max_per_img kept.
      view_dets, flips, widths, max_per_img   as tta_merge
      wbf          dict(iou_threshold, skip_box_thr, conf_type 'avg' | 'max', weights: one per view); None: WBF
    -> WbfDetections over [N, K] rows (K = max_per_img, or V * Q): `index` is the c = v * Q + j of every row's founder,
    `votes` its number of members; `detections_to_host` fetches all of it in one copy."""
    w = wbf_settings(wbf)
    dtype, dev, N, V, Q, boxes, scores, labels, count, flips, widths = _merge_operands("wbf_merge", view_dets, flips, widths)
    if V * Q > WBF_MAX_CANDIDATES:
        raise ValueError(f"wbf_merge: at most {WBF_MAX_CANDIDATES} candidates per image, got {V} views of {Q}")
    if w["weights"] is not None and len(w["weights"]) != V:
        raise ValueError(f"wbf_merge: {V} views but {len(w['weights'])} weights")
    keep, out = _merged_result(N, V, Q, dtype, dev, max_per_img, Q == 0, votes=True)
    if Q == 0:
        return out
    with torch.cuda.device(dev):
        _wbf.wbf_merge(boxes.view(V, N, Q, 4), scores.view(V, N, Q), labels.view(V, N, Q), count.view(V, N),
                       sum(1 << v for v, f in enumerate(flips) if f), widths.to(dev, torch.float32).contiguous(),
                       w["weights"], _wbf.CONF_TYPES[w["conf_type"]], w["iou_threshold"], w["skip_box_thr"], keep,
                       out.boxes, out.scores, out.labels, out.index, out.count, out.votes)
    return out


def weighted_boxes_fusion(boxes_list, scores_list, labels_list, weights=None, iou_thr=0.55, skip_box_thr=0.0,
                          conf_type="avg"):
    """`ensemble_boxes.weighted_boxes_fusion`'s call shape for one image, the counterpart of `soft_nms`: one entry per
    model (or view) in each list -- boxes [n_i, 4], scores [n_i], labels [n_i], tensors on the GPU or array-likes; pixel
    or normalised coordinates -- `weights` one per entry.  -> (boxes [E, 4], scores [E], labels [E] int64) in descending
    score order, fp32 on the GPU.  The ragged lists are padded into the [V, 1, Q] operands of one wbf_merge launch; the
    rule and its deviations from the package are include/codetr_wbf.h's (parity is unpinned)."""
    V = len(scores_list)
    if V == 0 or len(boxes_list) != V or len(labels_list) != V:
        raise ValueError("weighted_boxes_fusion: boxes_list, scores_list and labels_list of one length > 0")
    dev = next((t.device for t in scores_list if torch.is_tensor(t) and t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    sc = [torch.as_tensor(s, dtype=torch.float32).reshape(-1).to(dev) for s in scores_list]
    bx = [torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4).to(dev) for b in boxes_list]
    lb = [torch.as_tensor(l).reshape(-1).to(dev, torch.int64) for l in labels_list]
    if any(b.shape[0] != s.shape[0] or l.shape[0] != s.shape[0] for b, s, l in zip(bx, sc, lb)):
        raise ValueError("weighted_boxes_fusion: every entry n boxes [n, 4], n scores and n labels")
    Q = max(s.shape[0] for s in sc)
    if Q == 0:
        return (torch.zeros((0, 4), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.float32, device=dev),
                torch.zeros((0,), dtype=torch.int64, device=dev))
    boxes = torch.zeros((V, Q, 4), dtype=torch.float32, device=dev)
    scores = torch.zeros((V, Q), dtype=torch.float32, device=dev)
    labels = torch.zeros((V, Q), dtype=torch.int64, device=dev)
    for v in range(V):
        n = sc[v].shape[0]
        boxes[v, :n], scores[v, :n], labels[v, :n] = bx[v], sc[v], lb[v]
    count = torch.tensor([s.shape[0] for s in sc], dtype=torch.int32, device=dev)
    dets = wbf_merge([Detections(boxes, scores, labels, count, None)], [False] * V, [0.0],
                     dict(iou_threshold=iou_thr, skip_box_thr=skip_box_thr, conf_type=conf_type,
                          weights=None if weights is None else list(weights)))
    c = int(dets.count[0])
    return dets.boxes[0, :c], dets.scores[0, :c], dets.labels[0, :c]


SLICE_MAX_VIEWS = _cabi.SLICE_MAX_VIEWS
SLICE_MERGE = dict(type="nmm", metric="ios", threshold=0.5, class_agnostic=False)   # SAHI's defaults


def slice_merge_settings(merge=None):
    """the `merge` dict of sliced inference, validated and completed from SLICE_MERGE -> dict(type 'nmm' | 'nms',
    metric 'ios' | 'iou', threshold, class_agnostic)"""
    return _check.validated("slice merge", SLICE_MERGE, merge, dict(
        type=_check.one_of(_cabi.SLICE_MODES), metric=_check.one_of(_cabi.SLICE_METRICS),
        threshold=_check.number(coerce=True), class_agnostic=bool))


def slice_merge(dets, rows, origins, sizes, merge=None, max_per_img=None):
    """The fusion of sliced inference's per-tile detections for N images in one launch (csrc/prepost.hip; semantics:
    include/codetr_hip.h): every row's boxes shifted by its tile's origin and clipped to the image, then per label (or
    over all labels) greedy NMS, or greedy non-maximum merging in which a pick absorbs what it retires into the box
    around them, under IoU or IoS (intersection over the smaller area); the best max_per_img kept.
      dets         the results of postprocess_detections / postprocess_detections_soft over R rows (one entry, or a
                   list concatenated in order), boxes in each crop's own pixel coordinates
      rows         [N, V] int32: the row of image n's v-th view; a value outside [0, R) is an absent view
      origins      [R, 2] fp32 (x0, y0) of every row's crop;  sizes  [N, 2] fp32 (W, H) of the original images
                   (tensors on the device, or nested lists)
      merge        dict(type 'nmm' | 'nms', metric 'ios' | 'iou', threshold, class_agnostic); None: SLICE_MERGE
      max_per_img  None: all
    -> SoftDetections over [N, K] rows (K = max_per_img, or V * Q): `index` is c = v * Q + j of every row (of the pick, in
    'nmm'); `detections_to_host` fetches all of it in one copy."""
    m = slice_merge_settings(merge)
    dets, dtype, dev, Q = _entries("slice_merge", dets)
    R = sum(d.scores.shape[0] for d in dets)
    rows = torch.as_tensor(rows, dtype=torch.int32)
    origins = torch.as_tensor(origins, dtype=torch.float32)
    sizes = torch.as_tensor(sizes, dtype=torch.float32)
    if rows.dim() != 2 or rows.numel() == 0 or tuple(origins.shape) != (R, 2) or tuple(sizes.shape) != (rows.shape[0], 2):
        raise ValueError("slice_merge: rows [N, V], origins [R, 2], sizes [N, 2] with N, V > 0")
    N, V = rows.shape
    if V > SLICE_MAX_VIEWS or V * Q > TTA_MAX_CANDIDATES:
        raise ValueError(f"slice_merge: at most {SLICE_MAX_VIEWS} views and {TTA_MAX_CANDIDATES} candidates per image, "
                         f"got {V} views of {Q}")
    boxes, scores, labels, count = _cat(dets)
    keep, out = _merged_result(N, V, Q, dtype, dev, max_per_img, Q == 0 or R == 0)
    if Q == 0 or R == 0:
        return out
    with torch.cuda.device(dev):
        _cabi.slice_merge(boxes, scores, labels, count, rows.to(dev).contiguous(), origins.to(dev).contiguous(),
                          sizes.to(dev).contiguous(), _cabi.SLICE_METRICS[m["metric"]], _cabi.SLICE_MODES[m["type"]],
                          m["threshold"], m["class_agnostic"], keep, out.boxes, out.scores, out.labels, out.index,
                          out.count)
    return out

