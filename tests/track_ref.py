"""The tracking rule of include/codetr_hip.h ("Tracking") restated in numpy: float32 scalars, one operation per line
(the pair values of an association as elementwise float32 arrays: the same roundings), the greedy association with the
stated ties.  `TrackRef` is one stream's state; `update(boxes, scores, labels, count)`
is one frame and returns the id of every row.  The tests compare the kernel's ids and its decoded state with this bit
for bit; `tools/bench_inferencer.py --track` uses it as the host composition the kernel replaces."""
import collections

import numpy as np

F = np.float32
WP = F(1.0) / F(20.0)
WV = F(1.0) / F(160.0)

DEFAULTS = dict(obj_score_thrs=dict(high=0.6, low=0.1), init_track_thr=0.7, weight_iou_with_det_scores=True,
                match_iou_thrs=dict(high=0.1, low=0.5, tentative=0.3), num_frames_retain=30, num_tentatives=3,
                max_tracks=256)

State = collections.namedtuple("State", "f next_id refused id label hits tentative last mean cov")


def widen(x):
    """fp16 / bf16 / fp32 values (numpy array, or torch tensor on the host) -> float32 numpy, exactly"""
    if hasattr(x, "detach"):
        import torch
        if x.dtype == torch.bfloat16:   # (numpy has no bf16: the bits, shifted)
            return (x.contiguous().view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
        x = x.numpy()
    return np.asarray(x).astype(np.float32)


def std_p(c, h):
    return F(1e-2) if c == 2 else WP * h


def std_v(c, h):
    return F(1e-5) if c == 2 else WV * h


def measurement(box):
    x1, y1, x2, y2 = (F(v) for v in box)
    h = y2 - y1
    sx = x1 + x2
    sy = y1 + y2
    w = x2 - x1
    return [sx * F(0.5), sy * F(0.5), w / h, h]


def area(b):
    w = b[2] - b[0]
    h = b[3] - b[1]
    return w * h


def iou(bk, bc):
    """the library's IoU of two boxes (x1, y1, x2, y2) of float32 scalars"""
    iw = np.fmax(F(0), np.fmin(bk[2], bc[2]) - np.fmax(bk[0], bc[0]))
    ih = np.fmax(F(0), np.fmin(bk[3], bc[3]) - np.fmax(bk[1], bc[1]))
    inter = iw * ih
    uni = area(bk) + area(bc)
    return inter / (uni - inter)


class TrackRef:
    def __init__(self, settings=None):
        s = dict(DEFAULTS)
        s.update(settings or {})
        self.obj_high, self.obj_low = F(s["obj_score_thrs"]["high"]), F(s["obj_score_thrs"]["low"])
        self.init_thr = F(s["init_track_thr"])
        self.weight = bool(s["weight_iou_with_det_scores"])
        m = s["match_iou_thrs"]
        self.m_high, self.m_low, self.m_tent = F(m["high"]), F(m["low"]), F(m["tentative"])
        self.retain, self.tentatives, self.T = int(s["num_frames_retain"]), int(s["num_tentatives"]), int(s["max_tracks"])
        T = self.T
        self.f, self.issued, self.refused = 0, 0, 0
        self.id = np.zeros(T, np.int32)
        self.label = np.zeros(T, np.int64)
        self.hits = np.zeros(T, np.int32)
        self.tent = np.zeros(T, np.int32)
        self.last = np.zeros(T, np.int32)
        self.mean = np.zeros((T, 4, 2), np.float32)
        self.cov = np.zeros((T, 4, 3), np.float32)
        self.log = collections.Counter()   # which branches a sequence took: the tests assert on it

    def state(self):
        return State(self.f, self.issued + 1, self.refused, self.id.copy(), self.label.copy(), self.hits.copy(),
                     self.tent.copy(), self.last.copy(), self.mean.copy(), self.cov.copy())

    # ---- the filter -----------------------------------------------------------------------------------
    def initiate(self, t, z):
        zh = z[3]
        for c in range(4):
            if c == 2:
                sp, sv = F(1e-2), F(1e-5)
            else:
                sp = F(2.0) * (WP * zh)
                sv = F(10.0) * (WV * zh)
            self.mean[t, c] = (z[c], F(0))
            self.cov[t, c] = (sp * sp, F(0), sv * sv)

    def predict(self, t):
        h = self.mean[t, 3, 0]
        for c in range(4):
            p, v = self.mean[t, c]
            A, B, C = self.cov[t, c]
            sp, sv = std_p(c, h), std_v(c, h)
            a1 = A + F(2.0) * B
            a2 = a1 + C
            self.mean[t, c, 0] = p + v
            self.cov[t, c] = (a2 + sp * sp, B + C, C + sv * sv)

    def correct(self, t, z):
        h = self.mean[t, 3, 0]
        for c in range(4):
            p, v = self.mean[t, c]
            A, B, C = self.cov[t, c]
            sr = F(1e-1) if c == 2 else WP * h
            S = A + sr * sr
            k0 = A / S
            k1 = B / S
            y = z[c] - p
            self.mean[t, c] = (p + k0 * y, v + k1 * y)
            self.cov[t, c] = (A - k0 * A, B - k0 * B, C - k1 * B)

    def box(self, t):
        cx, cy, a, h = self.mean[t, :, 0]
        w = a * h
        hw = w * F(0.5)
        hh = h * F(0.5)
        return (cx - hw, cy - hh, cx + hw, cy + hh)

    # ---- one greedy association -------------------------------------------------------------------------
    def greedy(self, tracks, cands, boxes, scores, labels, match, free, weighted, thr, tag):
        """the values of all pairs at once (elementwise float32: the same roundings as pair by pair), then pick by pick"""
        if not tracks or not cands:
            return
        tb = np.array([self.box(t) for t in tracks], np.float32)[:, None, :]   # [nt, 1, 4]
        cb = boxes[cands][None, :, :]                                            # [1, nc, 4]
        iw = np.fmin(tb[..., 2], cb[..., 2]) - np.fmax(tb[..., 0], cb[..., 0])
        iw = np.fmax(F(0), iw)
        ih = np.fmin(tb[..., 3], cb[..., 3]) - np.fmax(tb[..., 1], cb[..., 1])
        ih = np.fmax(F(0), ih)
        inter = iw * ih
        at = (tb[..., 2] - tb[..., 0]) * (tb[..., 3] - tb[..., 1])
        ac = (cb[..., 2] - cb[..., 0]) * (cb[..., 3] - cb[..., 1])
        uni = at + ac
        val = inter / (uni - inter)
        if weighted:
            val = val * scores[cands][None, :]
        assert val.dtype == np.float32
        ok = (val >= thr) & (labels[cands][None, :] == self.label[tracks][:, None])   # (a NaN compares false)
        ok &= free[cands][None, :]                 # (a candidate an earlier association took is out)
        while ok.any():
            v = np.where(ok, val, F(-np.inf))
            k = int(np.argmax(v))                  # the first of the maxima in row-major order: lowest slot, then lowest j
            if int((v == v.flat[k]).sum()) > 1:
                self.log["tie"] += 1
            ti, ji = divmod(k, len(cands))
            match[tracks[ti]] = cands[ji]
            free[cands[ji]] = False
            ok[ti, :] = False
            ok[:, ji] = False
            self.log[tag] += 1

    # ---- one frame --------------------------------------------------------------------------------------
    def update(self, boxes, scores, labels, count=None):
        """boxes [Q, 4], scores [Q] (any float dtype: widened exactly), labels [Q]; rows >= count take no part -> [Q] int32"""
        with np.errstate(all="ignore"):
            return self._update(widen(boxes), widen(scores), np.asarray(labels).astype(np.int64), count)

    def _update(self, boxes, scores, labels, count):
        Q = scores.shape[0]
        cnt = Q if count is None else min(max(int(count), 0), Q)
        f, T = self.f, self.T
        out = np.zeros(Q, np.int32)
        high, low = [], []
        for j in range(cnt):
            b, sc = boxes[j], scores[j]
            if not (np.isfinite(b).all() and np.isfinite(sc)) or not b[2] - b[0] > 0 or not b[3] - b[1] > 0:
                continue
            if sc > self.obj_high:
                high.append(j)
            elif sc > self.obj_low:
                low.append(j)
        live = [t for t in range(T) if self.id[t] != 0]
        for t in live:
            if self.last[t] != f - 1:
                self.mean[t, 3, 1] = F(0)
            self.predict(t)
        match = np.full(T, -1, np.int64)
        free = np.zeros(Q, bool)
        free[high + low] = True
        conf = [t for t in live if not self.tent[t]]
        tent = [t for t in live if self.tent[t]]
        self.greedy(conf, high, boxes, scores, labels, match, free, self.weight, self.m_high, "A")
        self.greedy(tent, high, boxes, scores, labels, match, free, self.weight, self.m_tent, "B")
        recent = [t for t in conf if match[t] < 0 and self.last[t] == f - 1]
        self.greedy(recent, low, boxes, scores, labels, match, free, False, self.m_low, "C")
        for t in live:
            j = match[t]
            if j >= 0:
                self.correct(t, measurement(boxes[j]))
                self.last[t] = f
                self.hits[t] += 1
                self.label[t] = labels[j]
                if self.tent[t] and self.hits[t] >= self.tentatives:
                    self.tent[t] = 0
                    self.log["promoted"] += 1
                out[j] = -self.id[t] if self.tent[t] else self.id[t]
            elif self.tent[t] or f - self.last[t] >= self.retain:
                self.log["tentative_removed" if self.tent[t] else "retired"] += 1
                self.id[t] = self.hits[t] = self.tent[t] = self.last[t] = 0
                self.label[t] = 0
                self.mean[t] = 0
                self.cov[t] = 0
        for j in high:
            if not free[j] or not scores[j] > self.init_thr:
                continue
            slots = np.flatnonzero(self.id == 0)
            if slots.size == 0:
                self.refused += 1
                self.log["refused"] += 1
                continue
            t = int(slots[0])
            self.issued += 1
            self.id[t], self.hits[t], self.tent[t], self.last[t] = self.issued, 1, int(f != 0), f
            self.label[t] = labels[j]
            self.initiate(t, measurement(boxes[j]))
            out[j] = -self.id[t] if self.tent[t] else self.id[t]
            self.log["started"] += 1
        self.f = f + 1
        return out
