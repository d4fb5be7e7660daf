"""CPU reference of the test-time-augmentation merge (helper code for tests/test_tta_*.py, not collected by pytest).

`merge` restates, in numpy fp32 with one rounding per operation, the semantics include/codetr_hip.h gives for
codetr_tta_merge_*: the candidates of V views (rows j < count[v] of view v; candidate index c = v * Q + j), a flipped
view's box un-flipped to (W - x2, y1, W - x1, y2), then per label either hard NMS -- the greedy pick (highest score, ties
to the lowest c) retires every alive candidate with IoU > threshold -- or the soft-NMS of softnms_ref.soft_nms over the
concatenated candidates, the emitted detections sorted by (decayed) score with ties by ascending c, cut to max_keep.
`merge_outputs` adds the rounding to the storage type, i.e. the kernel's outputs for one image.
"""
import numpy as np

import softnms_ref

F = np.float32


def unflip(boxes, width):
    """(W - x2, y1, W - x1, y2) in fp32, one rounding per coordinate"""
    b = np.asarray(boxes, F)
    out = b.copy()
    out[..., 0] = F(width) - b[..., 2]
    out[..., 2] = F(width) - b[..., 0]
    return out


def hard_nms(boxes, scores, labels, iou_threshold, max_keep=0):
    """per-label greedy hard NMS in softnms_ref's arithmetic -> (index [E] int64, scores [E] fp32) in output order"""
    boxes, scores, labels = np.asarray(boxes, F), np.asarray(scores, F), np.asarray(labels)
    thr = F(iou_threshold)
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    out = []
    for lab in np.unique(labels):
        idx = np.flatnonzero(labels == lab)               # ascending candidate index
        b, a, s = boxes[idx], areas[idx], scores[idx]
        alive = np.ones(len(idx), bool)
        while True:
            k = softnms_ref._best(s, alive)
            if k < 0:
                break
            out.append(int(idx[k]))
            alive[k] = False
            with np.errstate(invalid="ignore"):
                alive &= ~(softnms_ref._overlaps(b[k], a[k], b, a) > thr)   # NaN compares false: kept
    out_idx = np.asarray(out, np.int64)
    out_sc = scores[out_idx] if len(out_idx) else np.zeros((0,), F)
    if len(out_idx):
        key = (softnms_ref.score_keys(out_sc) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - out_idx.astype(np.uint64))
        order = np.argsort(key, kind="stable")[::-1]
        out_idx, out_sc = out_idx[order], out_sc[order]
    if max_keep > 0:
        out_idx, out_sc = out_idx[:max_keep], out_sc[:max_keep]
    return out_idx, out_sc


def merge(boxes, scores, labels, count, flips, width, mode="nms", iou_threshold=0.5, min_score=1e-3, max_keep=0):
    """one image: boxes [V,Q,4], scores [V,Q] (fp32 values of the storage type), labels [V,Q], count [V], flips [V]
    bool, width the original image width; mode 'nms' | 'naive' | 'linear'.
    -> (c [E] int64, scores [E] fp32, boxes [E,4] fp32 un-flipped) in output order"""
    assert mode in ("nms", "naive", "linear")
    boxes, scores, labels = np.asarray(boxes, F), np.asarray(scores, F), np.asarray(labels)
    V, Q = scores.shape
    ub = np.stack([unflip(boxes[v], width) if flips[v] else boxes[v] for v in range(V)]).reshape(V * Q, 4)
    cand = np.flatnonzero((np.arange(Q)[None, :] < np.asarray(count).reshape(V, 1)).reshape(-1))   # ascending c
    b, s, lab = ub[cand], scores.reshape(-1)[cand], labels.reshape(-1)[cand]
    if len(cand) == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), F), np.zeros((0, 4), F)
    if mode == "nms":
        idx, sc = hard_nms(b, s, lab, iou_threshold, max_keep)
    else:
        idx, sc = softnms_ref.soft_nms(b, s, lab, iou_threshold, mode, min_score, None, max_keep)
    return cand[idx], sc, b[idx]


def merge_outputs(boxes, scores, labels, count, flips, width, to_storage, mode="nms", iou_threshold=0.5, min_score=1e-3,
                  max_keep=0):
    """the kernel's outputs for one image: (boxes [E,4], scores [E]) through `to_storage` (fp32 array -> the storage
    type, one rounding), labels [E], index [E]"""
    c, sc, bx = merge(boxes, scores, labels, count, flips, width, mode, iou_threshold, min_score, max_keep)
    return to_storage(bx.reshape(-1, 4)), to_storage(sc), np.asarray(labels).reshape(-1)[c], c
