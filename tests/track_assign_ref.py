"""The tracker of include/codetr_assign.h (association = optimal) restated in numpy: `TrackRef` with its three greedy
associations replaced by the assignment procedure of `assign_ref` over the integer gains the header states.  Everything
else -- candidates, filters, retirement, starts -- is `TrackRef`'s.  `log["rounds"]` sums the solver's rounds."""
import numpy as np

import assign_ref
from track_ref import F, TrackRef


def gains(val, thr):
    """float32 values -> the integer gains of the pairs with value >= thr (0 elsewhere, a NaN included)"""
    with np.errstate(all="ignore"):
        d = np.fmin(val - thr, F(2.0)) * F(1048576.0)
        assert d.dtype == np.float32
        ok = val >= thr
        return np.where(ok, 1 + np.where(ok, d, F(0)).astype(np.int64), 0)


class TrackAssignRef(TrackRef):
    def _update(self, boxes, scores, labels, count):
        Q = scores.shape[0]
        self._cnt = Q if count is None else min(max(int(count), 0), Q)   # the columns are all candidate rows
        return super()._update(boxes, scores, labels, count)

    def greedy(self, tracks, cands, boxes, scores, labels, match, free, weighted, thr, tag):
        """one association: the pair values exactly as TrackRef computes them, then the assignment"""
        if not tracks or not cands:
            return
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
        val = inter / (uni - inter)
        if weighted:
            val = val * scores[cands][None, :]
        assert val.dtype == np.float32
        g = gains(val, thr)
        g[labels[cands][None, :] != self.label[tracks][:, None]] = 0
        g[:, ~free[cands]] = 0
        rows = np.flatnonzero(g.any(axis=1))          # the tracks with at least one eligible pair, ascending slot
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
                self.log[tag] += 1
