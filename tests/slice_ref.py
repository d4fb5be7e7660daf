"""CPU reference of sliced inference (helper code for tests/test_slice_*.py, not collected by pytest).

`merge` restates, in numpy fp32 with one rounding per operation, the semantics include/codetr_hip.h gives for
codetr_slice_merge_*: the candidates of an image's V views (rows j < count[row] of the view's row; candidate index
c = v * Q + j), every box shifted by its row's origin and clipped to the image (np.fmax / np.fmin: a NaN coordinate
becomes 0, as fmaxf / fminf on the device), then per label -- or over all labels -- the greedy pick (highest score,
ties to the lowest c) that retires every alive candidate whose overlap with it is > threshold, the overlap being IoU or
IoS (intersection over the smaller area; the rounded product w * h is computed before anything is subtracted from or
divided by it).  In 'nmm' mode the pick's box becomes the box around itself and what it retired.  The emitted detections
are sorted by score with ties by ascending c and cut to max_keep.  `merge_outputs` adds the rounding to the storage
type, i.e. the kernel's outputs for one image.

`axis_starts` / `grid` restate the tile-grid rule of `Inferencer.slice_grid` independently of it.
"""
import numpy as np

import softnms_ref

F = np.float32


def axis_starts(L, t, o):
    """one axis of length L, tile t, overlap ratio o -> (starts, tile length)"""
    step = max(1, t - int(o * t))
    starts, p = [], 0
    while True:
        if p + t >= L:                     # the first tile to reach the end: moved back to end at L
            starts.append(max(0, L - t))
            return starts, min(t, L)
        starts.append(p)
        p += step


def grid(H, W, tile, overlap):
    """-> [(y0, x0, h, w)] y-major; tile (w, h), overlap (ox, oy)"""
    xs, w = axis_starts(W, tile[0], overlap[0])
    ys, h = axis_starts(H, tile[1], overlap[1])
    return [(y, x, h, w) for y in ys for x in xs]


def shift_clip(boxes, origin, size):
    """boxes [n, 4] of a crop at origin (x0, y0) -> in the (W, H) image: + origin, one rounding, then clipped"""
    b = np.asarray(boxes, F).reshape(-1, 4)
    off = np.asarray([origin[0], origin[1], origin[0], origin[1]], F)
    hi = np.asarray([size[0], size[1], size[0], size[1]], F)
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(b + off[None, :], F(0)), hi[None, :]).astype(F)


def overlaps(bk, ak, boxes, areas, metric):
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.maximum(F(0), np.minimum(bk[2], boxes[:, 2]) - np.maximum(bk[0], boxes[:, 0]))
        h = np.maximum(F(0), np.minimum(bk[3], boxes[:, 3]) - np.maximum(bk[1], boxes[:, 1]))
        inter = w * h                                      # the rounded product, before the subtraction
        if metric == "iou":
            return inter / ((ak + areas) - inter)
        return inter / np.fmin(ak, areas)


def greedy(boxes, scores, labels, metric="ios", mode="nmm", threshold=0.5, class_agnostic=False, max_keep=0):
    """boxes [n, 4] (already in image coordinates), scores [n], labels [n], n candidates in ascending c
    -> (position [E] int64, scores [E] fp32, boxes [E, 4] fp32) in output order"""
    assert metric in ("iou", "ios") and mode in ("nms", "nmm")
    boxes, scores, labels = np.asarray(boxes, F).reshape(-1, 4), np.asarray(scores, F), np.asarray(labels)
    thr = F(threshold)
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    seg = np.zeros(len(scores), np.int64) if class_agnostic else labels
    out, out_box = [], []
    for lab in np.unique(seg):
        idx = np.flatnonzero(seg == lab)
        b, a, s = boxes[idx], areas[idx], scores[idx]
        alive = np.ones(len(idx), bool)
        while True:
            k = softnms_ref._best(s, alive)
            if k < 0:
                break
            alive[k] = False
            with np.errstate(invalid="ignore"):
                hit = alive & (overlaps(b[k], a[k], b, a, metric) > thr)     # NaN compares false: kept
            alive &= ~hit
            box = b[k].copy()
            if mode == "nmm" and hit.any():                                    # against k's own box, never a grown one
                box = np.concatenate((np.minimum(box[:2], b[hit][:, :2].min(0)), np.maximum(box[2:], b[hit][:, 2:].max(0))))
            out.append(int(idx[k]))
            out_box.append(box.astype(F))
    pos = np.asarray(out, np.int64)
    if len(pos) == 0:
        return pos, np.zeros((0,), F), np.zeros((0, 4), F)
    sc, bx = scores[pos], np.stack(out_box)
    key = (softnms_ref.score_keys(sc) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - pos.astype(np.uint64))
    order = np.argsort(key, kind="stable")[::-1]
    pos, sc, bx = pos[order], sc[order], bx[order]
    if max_keep > 0:
        pos, sc, bx = pos[:max_keep], sc[:max_keep], bx[:max_keep]
    return pos, sc, bx


def merge(boxes, scores, labels, count, rows, origins, size, metric="ios", mode="nmm", threshold=0.5,
          class_agnostic=False, max_keep=0):
    """one image: boxes [R,Q,4], scores [R,Q] (fp32 values of the storage type), labels [R,Q], count [R]; rows [V]: the
    row of every view (outside [0, R): absent); origins [R,2] (x0, y0); size (W, H).
    -> (c [E] int64, scores [E] fp32, boxes [E,4] fp32, labels [E]) in output order"""
    boxes, scores, labels = np.asarray(boxes, F), np.asarray(scores, F), np.asarray(labels)
    R, Q = scores.shape
    cs, bs, ss, ls = [], [], [], []
    for v, r in enumerate(rows):
        r = int(r)
        if not 0 <= r < R:
            continue
        n = min(max(int(count[r]), 0), Q)
        cs.append(v * Q + np.arange(n, dtype=np.int64))
        bs.append(shift_clip(boxes[r, :n], origins[r], size))
        ss.append(scores[r, :n])
        ls.append(labels[r, :n])
    if not cs or sum(len(c) for c in cs) == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), F), np.zeros((0, 4), F), np.zeros((0,), np.int64)
    c, b, s, lab = np.concatenate(cs), np.concatenate(bs), np.concatenate(ss), np.concatenate(ls)
    pos, sc, bx = greedy(b, s, lab, metric, mode, threshold, class_agnostic, max_keep)
    return c[pos], sc, bx, lab[pos]


def merge_outputs(boxes, scores, labels, count, rows, origins, size, to_storage, **kw):
    """the kernel's outputs for one image: (boxes [E,4], scores [E]) through `to_storage` (fp32 array -> the storage
    type, one rounding), labels [E], index [E]"""
    c, sc, bx, lab = merge(boxes, scores, labels, count, rows, origins, size, **kw)
    return to_storage(bx.reshape(-1, 4)), to_storage(sc), lab, c
