"""The trackers of include/codetr_motion.h (codetr_track_update3_*) restated in numpy: `TrackRef` and the
optimal-association `TrackAssignRef` with the two additions of the rule in `predict` -- the row's camera motion, where it is
valid and finite, is added to the predicted cx and cy (one float32 addition each).  `update(..., motion=(dx, dy, valid))`."""
import numpy as np

from track_assign_ref import TrackAssignRef
from track_ref import F, TrackRef


class _Compensated:
    _shift = None

    def update(self, boxes, scores, labels, count=None, motion=None):
        self._shift = None
        if motion is not None:
            dx, dy, valid = (F(v) for v in motion[:3])
            if valid == F(1) and np.isfinite(dx) and np.isfinite(dy):
                self._shift = (dx, dy)
        return super().update(boxes, scores, labels, count)

    def predict(self, t):
        super().predict(t)
        if self._shift is not None:
            self.mean[t, 0, 0] = self.mean[t, 0, 0] + self._shift[0]
            self.mean[t, 1, 0] = self.mean[t, 1, 0] + self._shift[1]


class TrackMotionRef(_Compensated, TrackRef):
    pass


class TrackAssignMotionRef(_Compensated, TrackAssignRef):
    pass
