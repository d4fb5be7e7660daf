"""The appearance cue of include/codetr_appearance.h restated in numpy.  `describe(img, boxes, count)` is the descriptor
rule, sample by sample in float32 with one rounding per operation.  `TrackAppRef` (greedy) and `TrackAssignAppRef`
(optimal) add the rule to the trackers of track_motion_sim_ref.py (codetr_track_update4_*):
`update(boxes, scores, labels, count, motion=None, desc=None)` with `desc` [Q, 128] uint16, or None for the tracker as it is;
`g` [T, 128] uint16 is the stream's appearance state.  The tests compare ids, tracker states and `g` with the kernels bit
for bit."""
import numpy as np

import assign_ref
from track_assign_ref import TrackAssignRef, gains
from track_motion_sim_ref import _Similarity
from track_ref import F, TrackRef, widen

DEFAULTS = dict(appearance_thr=0.75, proximity_thr=0.5, reid_gate=1.5)
U = [F(6 * i + 19) / F(128) for i in range(16)]
V = [F(6 * j + 35) / F(256) for j in range(32)]


def participates(box):
    b = [F(v) for v in box]
    with np.errstate(all="ignore"):
        return bool(np.isfinite(b).all() and b[2] - b[0] > 0 and b[3] - b[1] > 0)


def describe(img, boxes, count=None):
    """img [H, W, 3] uint8, boxes [Q, 4] of any float type (widened exactly), count -> [Q, 128] uint16"""
    boxes = widen(boxes)
    H, W = img.shape[:2]
    Q = boxes.shape[0]
    cnt = Q if count is None else min(max(int(count), 0), Q)
    out = np.zeros((Q, 128), np.uint16)
    with np.errstate(all="ignore"):
        for q in range(cnt):
            if not participates(boxes[q]):
                continue
            x1, y1, x2, y2 = (F(v) for v in boxes[q])
            w, h = x2 - x1, y2 - y1
            xs = [x1 + w * u for u in U]
            ys = [y1 + h * v for v in V]
            px = [int(np.fmin(np.fmax(np.floor(x), F(0)), F(W - 1))) for x in xs]
            py = [int(np.fmin(np.fmax(np.floor(y), F(0)), F(H - 1))) for y in ys]
            pix = img[np.array(py)[:, None], np.array(px)[None, :]].astype(np.int64)    # [32, 16, 3]
            bins = (np.arange(32)[:, None] // 16) * 64 + (pix[..., 0] >> 6) * 16 + (pix[..., 1] >> 6) * 4 + (pix[..., 2] >> 6)
            out[q] = np.bincount(bins.ravel(), minlength=128).astype(np.uint16)
    return out


def similarity(g, d):
    """g [128] uint16 (sixteenths), d [.., 128] uint16 -> float32 s, exactly I / 8192"""
    inter = np.minimum(g.astype(np.int64), 16 * d.astype(np.int64)).sum(axis=-1)
    return inter.astype(np.float32) / F(8192)


class _Appearance:
    def __init__(self, settings=None, appearance=None):
        super().__init__(settings)
        a = dict(DEFAULTS)
        a.update(appearance or {})
        self.app_thr, self.app_prox, self.app_gate = F(a["appearance_thr"]), F(a["proximity_thr"]), F(a["reid_gate"])
        self.g = np.zeros((self.T, 128), np.uint16)
        self._desc = None

    def update(self, boxes, scores, labels, count=None, motion=None, desc=None):
        self._desc = None if desc is None else np.asarray(desc).view(np.uint16).reshape(-1, 128)
        self._high = {}
        before = self.id.copy()
        out = super().update(boxes, scores, labels, count, motion)
        if self._desc is None:
            return out
        d16 = 16 * self._desc.astype(np.int64)
        for t, j in self._high.items():          # step 6: matched to a high candidate
            if not self.g[t].any():
                self.g[t] = d16[j].astype(np.uint16)
                self.log["adopted"] += 1
            else:
                self.g[t] = ((7 * self.g[t].astype(np.int64) + d16[j] + 4) >> 3).astype(np.uint16)
        for t in range(self.T):
            if before[t] != 0 and self.id[t] != before[t]:    # step 7: freed (and perhaps started again)
                self.g[t] = 0
            if self.id[t] != 0 and self.id[t] != before[t]:   # step 8: started by the row that carries its id
                j = int(np.flatnonzero(np.abs(out) == self.id[t])[0])
                self.g[t] = d16[j].astype(np.uint16)
        return out

    def values(self, tracks, cands, boxes, scores, weighted):
        """the pair values of matches A and B: TrackRef's, plus the similarity where the rule adds it"""
        tb = np.array([self.box(t) for t in tracks], np.float32)[:, None, :]
        cb = boxes[cands][None, :, :]
        iw = np.fmin(tb[..., 2], cb[..., 2]) - np.fmax(tb[..., 0], cb[..., 0])
        iw = np.fmax(F(0), iw)
        ih = np.fmin(tb[..., 3], cb[..., 3]) - np.fmax(tb[..., 1], cb[..., 1])
        ih = np.fmax(F(0), ih)
        inter = iw * ih
        at = (tb[..., 2] - tb[..., 0]) * (tb[..., 3] - tb[..., 1])
        ac = (cb[..., 2] - cb[..., 0]) * (cb[..., 3] - cb[..., 1])
        uni = at + ac
        iou = inter / (uni - inter)
        val = iou * scores[cands][None, :] if weighted else iou
        near = iou >= self.app_prox                      # (a NaN compares false)
        ccx = (cb[..., 0] + cb[..., 2]) * F(0.5)
        ccy = (cb[..., 1] + cb[..., 3]) * F(0.5)
        g2 = self.app_gate * self.app_gate
        for k, t in enumerate(tracks):
            lost = not self.tent[t] and self.last[t] != self.f - 1
            if lost and self.app_gate > 0:
                cx, cy, a, hh = self.mean[t, :, 0]
                dx = ccx[0] - cx
                dy = ccy[0] - cy
                d2 = dx * dx + dy * dy
                wt = a * hh
                r2 = g2 * (wt * wt + hh * hh)
                inside = d2 <= r2
                if (inside & ~near[k]).any():
                    self.log["gated"] += 1
                near[k] |= inside
        s = np.stack([similarity(self.g[t], self._desc[cands]) for t in tracks])
        add = near & (s >= self.app_thr)
        out = val + np.where(add, s, F(0))
        assert out.dtype == np.float32 and iou.dtype == np.float32
        self.log["added"] += int(add.sum())
        return out

    def greedy(self, tracks, cands, boxes, scores, labels, match, free, weighted, thr, tag):
        if self._desc is None or tag == "C":
            return super().greedy(tracks, cands, boxes, scores, labels, match, free, weighted, thr, tag)
        if not tracks or not cands:
            return
        val = self.values(tracks, cands, boxes, scores, weighted)
        same = labels[cands][None, :] == self.label[tracks][:, None]
        if isinstance(self, TrackAssignRef):     # the assignment of track_assign_ref.py over the gains of `val`
            g = gains(val, thr)
            g[~same] = 0
            g[:, ~free[cands]] = 0
            rows = np.flatnonzero(g.any(axis=1))
            if rows.size == 0:
                return
            G = np.zeros((rows.size, self._cnt), np.int64)
            G[:, cands] = g[rows]
            m, _, rounds = assign_ref.solve(G)
            self.log["rounds"] += rounds
            self.log["problems"] += 1
            for k, j in enumerate(m):
                if j >= 0:
                    match[tracks[rows[k]]] = j
                    free[j] = False
                    self._high[tracks[rows[k]]] = int(j)
                    self.log[tag] += 1
            return
        ok = (val >= thr) & same & free[cands][None, :]      # the picks of track_ref.py
        while ok.any():
            v = np.where(ok, val, F(-np.inf))
            k = int(np.argmax(v))
            if int((v == v.flat[k]).sum()) > 1:
                self.log["tie"] += 1
            ti, ji = divmod(k, len(cands))
            match[tracks[ti]] = cands[ji]
            free[cands[ji]] = False
            self._high[tracks[ti]] = int(cands[ji])
            ok[ti, :] = False
            ok[:, ji] = False
            self.log[tag] += 1


class TrackAppRef(_Appearance, _Similarity, TrackRef):
    pass


class TrackAssignAppRef(_Appearance, _Similarity, TrackAssignRef):
    pass
