"""The similarity rule of include/codetr_motion.h (version 2, codetr_motion_estimate2_u8) restated in numpy on top of
tests/motion_ref.py: the votes are that file's, the search over the pairs of textured blocks and the refit are integers
(int64 arrays for the search, whose terms stay below 2^40 in the unreduced form the header states first; Python ints for the
refit's sums), and float32 appears at the four divisions only.  `MotionSimRef.estimate(image)` is one frame and returns
((dx, dy, valid, model, a, b, px, py), (k, blocks, textured, agreeing, pairs, inliers, i, j)); the state is MotionRef's."""
import numpy as np

import motion_ref
from motion_ref import BLOCK

F = np.float32
ZERO8 = (F(0),) * 8


def f32(i):
    """one conversion of an integer to float32, round to nearest even (|i| < 2^53: the way through a double is exact)"""
    assert abs(int(i)) < 2 ** 53
    return F(float(int(i)))


def search(g, V, R):
    """g [n, 2] block indices (bx, by) and V [n, 2] votes of the textured blocks in ascending block order ->
    (eligible pairs, inliers of the best pair, i, j, inlier mask [n] or None)"""
    n = len(g)
    g, V = np.asarray(g, np.int64).reshape(n, 2), np.asarray(V, np.int64).reshape(n, 2)
    P = 16 * (R + BLOCK * g + BLOCK // 2)
    Q = P + V
    ii, jj = np.triu_indices(n, 1)                                        # i ascending, then j ascending
    keep = ((g[jj] - g[ii]) ** 2).sum(1) >= 4
    ii, jj = ii[keep], jj[keep]
    if len(ii) == 0:
        return 0, 0, -1, -1, None
    d, e = P[jj] - P[ii], Q[jj] - Q[ii]
    dd, A = (d * d).sum(1), (d * e).sum(1)
    B = d[:, 0] * e[:, 1] - d[:, 1] * e[:, 0]
    u = P[None] - P[ii][:, None]                                          # [pairs, n, 2]
    w = Q[None] - Q[ii][:, None]
    perp = np.stack((-u[..., 1], u[..., 0]), -1)
    r = A[:, None, None] * u + B[:, None, None] * perp - dd[:, None, None] * w
    inl = (np.abs(r) <= 16 * dd[:, None, None]).all(-1)
    cnt = inl.sum(1)
    best = int(np.argmax(cnt))                                            # the first maximum: the lowest i, then the lowest j
    return len(ii), int(cnt[best]), int(ii[best]), int(jj[best]), inl[best]


def refit(g, V, R, mask, k):
    """the refit over the inliers -> (dx, dy, a, b, px, py) float32, or None where one of its four conditions fails"""
    sums = [0] * 7
    c = 0
    for (bx, by), (vx, vy), m in zip(g, V, mask):
        if not m:
            continue
        Px, Py = 16 * (R + BLOCK * int(bx) + 8), 16 * (R + BLOCK * int(by) + 8)
        Qx, Qy = Px + int(vx), Py + int(vy)
        c += 1
        for s, v in enumerate((Px, Py, Qx, Qy, Px * Px + Py * Py, Px * Qx + Py * Qy, Px * Qy - Py * Qx)):
            sums[s] += v
    spx, spy, sqx, sqy, pp, pq, cross = sums
    Sxx = c * pp - (spx * spx + spy * spy)
    An = c * pq - (spx * sqx + spy * sqy)
    Bn = c * cross - (spx * sqy - spy * sqx)
    if not (Sxx > 0 and 2 * An >= Sxx and An <= 2 * Sxx and 2 * abs(Bn) <= Sxx):
        return None
    den = f32(16 * c)
    return (f32((sqx - spx) * k) / den, f32((sqy - spy) * k) / den, f32(An) / f32(Sxx), f32(Bn) / f32(Sxx),
            f32(spx * k) / den, f32(spy * k) / den)


def frame_motion(P, C, k, settings):
    """previous and current thumbnails of one size -> (motion8, (textured, agreeing, pairs, inliers, i, j))"""
    R = settings["search"]
    V = []
    (dx, dy, valid), (n, c) = motion_ref.frame_motion(P, C, k, settings, votes_out=V)
    nby, nbx = motion_ref.block_counts(P.shape[0], P.shape[1], R)
    g = [(bx, by) for by in range(nby) for bx in range(nbx)
         if motion_ref.textured(P[R + BLOCK * by:R + BLOCK * by + BLOCK, R + BLOCK * bx:R + BLOCK * bx + BLOCK],
                                settings["texture"])]
    assert len(g) == len(V) == n
    pairs, c2, i, j, mask = search(g, V, R)
    diag = (n, c, pairs, c2, i, j)
    mb = settings["min_blocks"]
    if n >= mb and pairs >= 1 and c2 >= mb and 2 * c2 >= n:
        fit = refit(g, V, R, mask, k)
        if fit is not None:
            return (fit[0], fit[1], F(1), F(2)) + fit[2:], diag
    if valid == 1:
        return (dx, dy, F(1), F(1), F(1), F(0), F(0), F(0)), diag
    return ZERO8, diag


class MotionSimRef(motion_ref.MotionRef):
    def estimate(self, image):
        H, W = image.shape[:2]
        k, C = motion_ref.thumbnail(image, self.settings["grid"])
        nby, nbx = motion_ref.block_counts(C.shape[0], C.shape[1], self.settings["search"])
        motion, rest = ZERO8, (0, 0, 0, 0, -1, -1)
        if self.have and (self.H, self.W, self.k) == (H, W, k):
            motion, rest = frame_motion(self.thumb, C, k, self.settings)
        self.have, self.H, self.W, self.k, self.thumb = 1, H, W, k, C
        return motion, (k, nby * nbx) + rest


def transform(motion):
    """the eight floats -> the 2 x 3 matrix [[a, -b, tx], [b, a, ty]] in float64 (nested lists), [[1, 0, dx], [0, 1, dy]]
    for a translation row, None for an invalid one: what the Inferencer reports as camera_transform"""
    dx, dy, valid, model, a, b, px, py = (float(v) for v in motion)
    if valid != 1.0:
        return None
    if model != 2.0:
        return [[1.0, 0.0, dx], [0.0, 1.0, dy]]
    return [[a, -b, (px + dx) - (a * px - b * py)], [b, a, (py + dy) - (b * px + a * py)]]
