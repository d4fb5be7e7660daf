"""The camera-motion rule of include/codetr_motion.h restated in numpy: integers, one float32 division per axis at the
end.  `MotionRef` is one stream's state; `estimate(image)` is one frame and returns ((dx, dy, valid), (k, blocks,
textured, agreeing)); `state_bytes()` is the state as the device keeps it.  The tests compare the kernels' motion floats,
diag ints and state bytes with this bit for bit."""
import numpy as np

DEFAULTS = dict(grid=160, search=8, texture=2, min_blocks=4)
BLOCK = 16
SIDE = 160


def thumbnail(image, grid):
    """[H, W, 3] uint8 -> (k, [th, tw] uint8)"""
    H, W = image.shape[:2]
    k = max(1, -(-max(H, W) // grid))
    th, tw = H // k, W // k
    px = image[:th * k, :tw * k].astype(np.int64)
    gray = (77 * px[..., 0] + 150 * px[..., 1] + 29 * px[..., 2] + 128) >> 8
    sums = gray.reshape(th, k, tw, k).sum(axis=(1, 3))
    return k, ((sums + (k * k) // 2) // (k * k)).astype(np.uint8)


def block_counts(th, tw, R):
    return max(0, (th - 2 * R) // BLOCK), max(0, (tw - 2 * R) // BLOCK)


def textured(block, texture):
    b = block.astype(np.int64)
    return int(np.abs(b[:, :-1] - b[:, 1:]).sum() + np.abs(b[:-1, :] - b[1:, :]).sum()) >= texture * 256


def sads(P, C, R, by, bx):
    """S[dy + R, dx + R] of block (by, bx): int64 [2 R + 1, 2 R + 1]"""
    block = P[R + BLOCK * by:R + BLOCK * by + BLOCK, R + BLOCK * bx:R + BLOCK * bx + BLOCK].astype(np.int64)
    region = C[BLOCK * by:BLOCK * by + BLOCK + 2 * R, BLOCK * bx:BLOCK * bx + BLOCK + 2 * R].astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(region, (BLOCK, BLOCK))
    return np.abs(win - block).sum(axis=(2, 3))


def step(sm, s0, sp):
    den = sm - 2 * s0 + sp
    if den <= 0:
        return 0
    return min(max((16 * (sm - sp) + den) // (2 * den), -8), 8)   # (Python's // is the floor division of the rule)


def vote(S, R):
    """the best displacement by (S, dy^2 + dx^2, dy, dx) and its sub-cell steps -> (vx, vy) in sixteenths of a cell"""
    S = S.astype(np.int64)
    cands = [(int(S[i, j]), (i - R) ** 2 + (j - R) ** 2, i - R, j - R) for i, j in np.argwhere(S == S.min())]
    s0, _, dy, dx = min(cands)
    i, j = dy + R, dx + R
    sx = step(int(S[i, j - 1]), s0, int(S[i, j + 1])) if 1 <= j <= 2 * R - 1 else 0
    sy = step(int(S[i - 1, j]), s0, int(S[i + 1, j])) if 1 <= i <= 2 * R - 1 else 0
    return 16 * dx + sx, 16 * dy + sy


def frame_motion(P, C, k, settings, votes_out=None):
    """previous and current thumbnails of one size -> ((dx, dy, valid), (textured, agreeing))"""
    R = settings["search"]
    nby, nbx = block_counts(P.shape[0], P.shape[1], R)
    votes = []
    for by in range(nby):
        for bx in range(nbx):
            blk = P[R + BLOCK * by:R + BLOCK * by + BLOCK, R + BLOCK * bx:R + BLOCK * bx + BLOCK]
            if textured(blk, settings["texture"]):
                votes.append(vote(sads(P, C, R, by, bx), R))
    if votes_out is not None:
        votes_out.extend(votes)
    n = len(votes)
    if n < settings["min_blocks"]:
        return (np.float32(0), np.float32(0), np.float32(0)), (n, 0)
    v = np.array(votes, np.int64)
    mx, my = np.sort(v[:, 0])[(n - 1) // 2], np.sort(v[:, 1])[(n - 1) // 2]
    agree = (np.abs(v[:, 0] - mx) <= 16) & (np.abs(v[:, 1] - my) <= 16)
    c = int(agree.sum())
    if 2 * c < n:
        return (np.float32(0), np.float32(0), np.float32(0)), (n, c)
    sx, sy = int(v[agree, 0].sum()), int(v[agree, 1].sum())
    dx = np.float32(np.int32(sx * k)) / np.float32(np.int32(16 * c))
    dy = np.float32(np.int32(sy * k)) / np.float32(np.int32(16 * c))
    return (dx, dy, np.float32(1)), (n, c)


class MotionRef:
    def __init__(self, settings=None):
        self.settings = dict(DEFAULTS)
        self.settings.update(settings or {})
        self.have, self.H, self.W, self.k, self.thumb = 0, 0, 0, 0, None

    def estimate(self, image):
        H, W = image.shape[:2]
        k, C = thumbnail(image, self.settings["grid"])
        nby, nbx = block_counts(C.shape[0], C.shape[1], self.settings["search"])
        motion, (n, c) = (np.float32(0), np.float32(0), np.float32(0)), (0, 0)
        if self.have and (self.H, self.W, self.k) == (H, W, k):
            motion, (n, c) = frame_motion(self.thumb, C, k, self.settings)
        self.have, self.H, self.W, self.k, self.thumb = 1, H, W, k, C
        return motion, (k, nby * nbx, n, c)

    def state_bytes(self):
        out = np.zeros(16 + SIDE * SIDE, np.uint8)
        out[:16] = np.array([self.have, self.H, self.W, self.k], np.int32).view(np.uint8)
        if self.thumb is not None:
            out[16:16 + self.thumb.size] = self.thumb.reshape(-1)
        return out
