"""The trackers of include/codetr_motion.h, version 2 (codetr_track_update4_*) restated in numpy: `TrackRef` and the
optimal-association `TrackAssignRef` with the header's `predict` -- by the row's model float the similarity about (px, py)
moves the predicted centre, its velocity and the height (float32, one rounding per operation in the header's order), or the
translation is added as codetr_track_update3_* adds it.  `update(..., motion=(dx, dy, valid, model, a, b, px, py))`."""
import numpy as np

from track_assign_ref import TrackAssignRef
from track_ref import F, TrackRef


class _Similarity:
    _row = None

    def update(self, boxes, scores, labels, count=None, motion=None):
        self._row = None
        if motion is not None:
            dx, dy, _, model, a, b, px, py = (F(v) for v in motion)
            if model == F(2) and all(np.isfinite(v) for v in (dx, dy, a, b, px, py)):
                with np.errstate(over="ignore"):
                    self._row = (2, a, b, px, py, px + dx, py + dy, np.sqrt(a * a + b * b, dtype=np.float32))
            elif model == F(1) and np.isfinite(dx) and np.isfinite(dy):
                self._row = (1, dx, dy)
        return super().update(boxes, scores, labels, count)

    def predict(self, t):
        super().predict(t)
        if self._row is None:
            return
        m = self.mean
        with np.errstate(over="ignore", invalid="ignore"):
            if self._row[0] == 1:
                m[t, 0, 0] = m[t, 0, 0] + self._row[1]
                m[t, 1, 0] = m[t, 1, 0] + self._row[2]
                return
            _, a, b, px, py, qx, qy, s = self._row
            ux, uy = m[t, 0, 0] - px, m[t, 1, 0] - py
            m[t, 0, 0] = qx + (a * ux - b * uy)
            m[t, 1, 0] = qy + (b * ux + a * uy)
            vx, vy = m[t, 0, 1], m[t, 1, 1]
            m[t, 0, 1] = a * vx - b * vy
            m[t, 1, 1] = b * vx + a * vy
            m[t, 3, 0] = m[t, 3, 0] * s
            m[t, 3, 1] = m[t, 3, 1] * s


class TrackMotionSimRef(_Similarity, TrackRef):
    pass


class TrackAssignMotionSimRef(_Similarity, TrackAssignRef):
    pass
