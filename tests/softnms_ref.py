"""CPU reference of the soft-NMS post-processing (helper code for tests/test_softnms_*.py, not collected by pytest).

`soft_nms` implements, in numpy fp32 with one rounding per operation, exactly the semantics that include/codetr_hip.h
states for codetr_postprocess_softnms_*: score threshold, the min_score pre-drop that spares the global maximum, the
per-label greedy loop (highest current score first, ties to the lowest query index; IoU >= threshold decays by 1 - IoU
(`linear`) or to 0 (`naive`); a score < min_score leaves), the final sort by decayed score (ties by ascending index) and
the max_keep cut.  `postprocess` adds the rescale and the rounding to the storage type, i.e. the kernel's outputs.

`soft_nms_literal` is a transcription of the sequential algorithm of mmcv 2.x's soft-NMS (softnms_cpu_kernel: select
the maximum of the rest, swap it to the front, decay everything behind it, swap-remove what falls under min_score) run
jointly over all classes with a class-aware weight (different label: weight 1), followed by batched_nms's sort by score.
PARITY UNPINNED: mmcv is not installed here, the transcription follows its published source; the two forms agree on
tie-free inputs (tests/test_softnms_cpu.py).  mmcv itself separates classes by adding label * (max + 1) to the
coordinates instead of comparing labels.
"""
import numpy as np

F = np.float32


def score_keys(scores):
    """the kernel's descending order of fp32 scores as uint64 keys: -0 is +0, a NaN with the sign bit clear is above
    +inf, one with it set below -inf (score_key of csrc/prepost.hip)"""
    s = np.asarray(scores, F).copy()
    s[s == 0] = 0.0
    u = s.view(np.uint32).astype(np.uint64)
    neg = (u & np.uint64(0x80000000)) != 0
    return np.where(neg, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def _best(scores, alive):
    """position of the highest current score among `alive`, ties to the lowest position; -1 if none"""
    if not alive.any():
        return -1
    n = len(scores)
    key = (score_keys(scores) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    key[~alive] = 0
    return int(np.argmax(key))


def _overlaps(bk, ak, boxes, areas):
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.maximum(F(0), np.minimum(bk[2], boxes[:, 2]) - np.maximum(bk[0], boxes[:, 0]))
        h = np.maximum(F(0), np.minimum(bk[3], boxes[:, 3]) - np.maximum(bk[1], boxes[:, 1]))
        inter = w * h
        return inter / ((ak + areas) - inter)


def soft_nms(boxes, scores, labels, iou_threshold, method="linear", min_score=1e-3, score_threshold=None, max_keep=0):
    """boxes [Q,4], scores [Q] (fp32 values of the storage type), labels [Q]; score_threshold already rounded to the
    storage type, or None.  -> (index [E] int64, decayed scores [E] fp32) in output order"""
    assert method in ("linear", "naive")
    boxes, scores, labels = np.asarray(boxes, F), np.asarray(scores, F).copy(), np.asarray(labels)
    Q = len(scores)
    thr, mn = F(iou_threshold), F(min_score)
    with np.errstate(invalid="ignore"):
        live = np.ones(Q, bool) if score_threshold is None else scores > F(score_threshold)
        g = _best(scores, live)
        low = scores < mn
    if g >= 0:
        low[g] = False
    live &= ~low
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    out_idx, out_sc = [], []
    for lab in np.unique(labels[live]):
        idx = np.flatnonzero(live & (labels == lab))      # ascending query index
        b, a, s = boxes[idx], areas[idx], scores[idx].copy()
        alive = np.ones(len(idx), bool)
        while True:
            k = _best(s, alive)
            if k < 0:
                break
            out_idx.append(int(idx[k]))
            out_sc.append(s[k])
            alive[k] = False
            ovr = _overlaps(b[k], a[k], b, a)
            with np.errstate(invalid="ignore"):
                hit = ovr >= thr                           # NaN compares false: weight 1
                weight = np.where(hit, (F(1) - ovr) if method == "linear" else F(0), F(1)).astype(F)
                s = np.where(alive, s * weight, s).astype(F)
                alive &= ~(s < mn)
    out_idx, out_sc = np.asarray(out_idx, np.int64), np.asarray(out_sc, F)
    if len(out_idx):
        key = (score_keys(out_sc) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - out_idx.astype(np.uint64))
        order = np.argsort(key, kind="stable")[::-1]      # keys are distinct (the index is part of them)
        out_idx, out_sc = out_idx[order], out_sc[order]
    if max_keep > 0:
        out_idx, out_sc = out_idx[:max_keep], out_sc[:max_keep]
    return out_idx, out_sc


def soft_nms_literal(boxes, scores, labels, iou_threshold, method="linear", min_score=1e-3):
    """mmcv's sequential loop over all classes at once -> (index, decayed scores) sorted by score descending"""
    assert method in ("linear", "naive")
    b = [np.asarray(r, F).copy() for r in np.asarray(boxes, F)]
    sc = [F(v) for v in np.asarray(scores, F)]
    lab = [int(v) for v in labels]
    ind = list(range(len(sc)))
    area = [F(F(r[2] - r[0]) * F(r[3] - r[1])) for r in b]
    thr, mn = F(iou_threshold), F(min_score)
    N = len(sc)

    def swap(i, j):
        for arr in (b, sc, lab, ind, area):
            arr[i], arr[j] = arr[j], arr[i]

    i = 0
    while i < N:
        max_pos = i
        for pos in range(i + 1, N):
            if sc[max_pos] < sc[pos]:
                max_pos = pos
        swap(i, max_pos)
        pos = i + 1
        while pos < N:
            w = max(F(0), F(min(b[i][2], b[pos][2]) - max(b[i][0], b[pos][0])))
            h = max(F(0), F(min(b[i][3], b[pos][3]) - max(b[i][1], b[pos][1])))
            inter = F(w * h)
            with np.errstate(invalid="ignore", divide="ignore"):
                ovr = F(inter / F(F(area[i] + area[pos]) - inter))
            weight = F(1)
            if lab[pos] == lab[i] and ovr >= thr:
                weight = F(1) - ovr if method == "linear" else F(0)
            sc[pos] = F(sc[pos] * weight)
            if sc[pos] < mn:
                swap(pos, N - 1)
                N -= 1
                pos -= 1
            pos += 1
        i += 1
    idx, s = np.asarray(ind[:N], np.int64), np.asarray(sc[:N], F)
    order = np.lexsort((idx, -s.astype(np.float64)))     # batched_nms: scores.argsort(descending=True)
    return idx[order], s[order]


def postprocess(boxes, scores, labels, divisors, to_storage, iou_threshold, method="linear", min_score=1e-3,
                score_threshold=None, max_keep=0):
    """one image's kernel outputs: (boxes [E,4], scores [E]) through `to_storage` (fp32 array -> the storage type, one
    rounding), labels [E], index [E].  boxes / scores / divisors hold fp32 values of the storage type."""
    idx, sc = soft_nms(boxes, scores, labels, iou_threshold, method, min_score, score_threshold, max_keep)
    with np.errstate(invalid="ignore", divide="ignore"):
        bx = np.asarray(boxes, F)[idx] / np.asarray(divisors, F)[None, :]
    return to_storage(bx.reshape(-1, 4)), to_storage(sc), np.asarray(labels)[idx], idx
