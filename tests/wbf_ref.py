"""CPU reference of weighted boxes fusion (helper code for tests/test_wbf_*.py, not collected by pytest).

`fuse` restates, in numpy fp32 with one rounding per operation, the rule include/codetr_wbf.h gives for
codetr_wbf_merge_*: the candidates of V views (rows j < count[v] of view v; candidate index c = v * Q + j), a flipped
view's box un-flipped, conf = score * weight[v], live iff score >= skip_box_thr and conf > 0; per label, in descending
conf (ties to the lowest c), a candidate joins the cluster whose fused box it overlaps most among those with
IoU > threshold (ties to the lowest founder c) or founds one; every cluster emits its fused box, score, founder and
votes; the rows sorted by score (ties by ascending founder c), cut to max_keep.  The loop over the clusters of a step is
vectorised (4096 candidates of one label are a second's work, not a minute's).  `fuse_outputs` adds the rounding to the
storage type, i.e. the kernel's outputs for one image.
"""
import numpy as np

import softnms_ref
import tta_ref

F = np.float32


def weight_sums(weights, V):
    """(weights [V] fp32, wsum: V rounded additions in view order starting from 0, wmax)"""
    w = np.ones(V, F) if weights is None else np.asarray(weights, F)
    assert w.shape == (V,)
    wsum = F(0)
    for x in w:
        wsum = F(wsum + x)
    return w, wsum, F(w.max())


def _keys(values, c):
    """(value, c) as one descending uint64 key: the higher value first, equal values in ascending c"""
    return (softnms_ref.score_keys(values) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(c).astype(np.uint64))


def fuse(boxes, scores, labels, count, flips, width, weights=None, conf_type="avg", iou_threshold=0.55,
         skip_box_thr=0.0, max_keep=0):
    """one image: boxes [V,Q,4], scores [V,Q] (fp32 values of the storage type), labels [V,Q], count [V], flips [V]
    bool, width the original image width.
    -> (boxes [E,4] fp32, scores [E] fp32, labels [E], index [E] int64 = the founders' c, votes [E] int64) in output order"""
    assert conf_type in ("avg", "max")
    boxes, scores, labels = np.asarray(boxes, F), np.asarray(scores, F), np.asarray(labels)
    V, Q = scores.shape
    w, wsum, wmax = weight_sums(weights, V)
    thr, skip = F(iou_threshold), F(skip_box_thr)
    ub = np.stack([tta_ref.unflip(boxes[v], width) if flips[v] else boxes[v] for v in range(V)]).reshape(V * Q, 4)
    conf = (scores * w[:, None]).astype(F).reshape(-1)
    flat_s, flat_l = scores.reshape(-1), labels.reshape(-1)
    with np.errstate(invalid="ignore"):
        live = (np.arange(Q)[None, :] < np.asarray(count).reshape(V, 1)).reshape(-1) & (flat_s >= skip) & (conf > 0)
    out_box, out_sc, out_c, out_n = [], [], [], []
    for lab in np.unique(flat_l[live]):
        idx = np.flatnonzero(live & (flat_l == lab))                      # ascending c
        order = idx[np.argsort(_keys(conf[idx], idx), kind="stable")[::-1]]   # conf descending, ties to the lowest c
        m = len(order)
        S, SC = np.zeros((m, 4), F), np.zeros(m, F)
        n, top, founder = np.zeros(m, np.int64), np.zeros(m, F), np.zeros(m, np.int64)
        K = 0
        for c in order:
            b, cf = ub[c], conf[c]
            j = -1
            if K:
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    Fk = S[:K] / SC[:K, None]
                    aF = (Fk[:, 2] - Fk[:, 0]) * (Fk[:, 3] - Fk[:, 1])
                    ovr = softnms_ref._overlaps(b, (b[2] - b[0]) * (b[3] - b[1]), Fk, aF)
                    hit = ovr > thr                                       # NaN compares false
                if hit.any():
                    key = _keys(ovr, founder[:K])
                    key[~hit] = 0
                    j = int(np.argmax(key))                               # highest ovr, ties to the lowest founder c
            with np.errstate(invalid="ignore", over="ignore"):
                if j < 0:
                    S[K], SC[K], n[K], top[K], founder[K] = cf * b, cf, 1, cf, c
                    K += 1
                else:
                    S[j] = S[j] + cf * b                                  # the product rounded, then the sum
                    SC[j] = SC[j] + cf
                    n[j] += 1
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            nf = n[:K].astype(F)
            sc = top[:K] / wmax if conf_type == "max" else ((SC[:K] / nf) * np.minimum(nf, wsum)) / wsum
            out_box.append(S[:K] / SC[:K, None])
        out_sc.append(sc.astype(F))
        out_c.append(founder[:K])
        out_n.append(n[:K])
    if not out_c:
        return np.zeros((0, 4), F), np.zeros((0,), F), np.zeros((0,), labels.dtype), np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    bx, sc, c, n = np.concatenate(out_box), np.concatenate(out_sc), np.concatenate(out_c), np.concatenate(out_n)
    order = np.argsort(_keys(sc, c), kind="stable")[::-1]
    if max_keep > 0:
        order = order[:max_keep]
    return bx[order], sc[order], flat_l[c[order]], c[order], n[order]


def fuse_outputs(boxes, scores, labels, count, flips, width, to_storage, **kw):
    """the kernel's outputs for one image: (boxes [E,4], scores [E]) through `to_storage` (fp32 array -> the storage
    type, one rounding), labels [E], index [E], votes [E]"""
    bx, sc, lab, c, n = fuse(boxes, scores, labels, count, flips, width, **kw)
    return to_storage(bx.reshape(-1, 4)), to_storage(sc), lab, c, n
