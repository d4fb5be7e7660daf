"""The rule of include/codetr_raw.h restated in numpy int64, step by step: normalise, pad by folding, slice arithmetic, table.
No tiling, nothing of the kernel's layout.  `real=True` is the same computation in float64 without any intermediate
rounding -- what the header's error bound is measured against."""
import numpy as np

PATTERNS = {"bayer_rggb": 0, "bayer_grbg": 1, "bayer_gbrg": 2, "bayer_bggr": 3}   # 2 ry + rx of the red site
LINEAR = ((np.arange(4096, dtype=np.int64) * 255 + 2047) // 4095).astype(np.uint8)


def multipliers(black, white, gains):
    return [int(np.floor(g * 4294901760.0 / float(white - black) + 0.5)) for g in gains]


def fold(i, n):
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def demosaic(s, pattern, bits=8, black_level=0, white_level=None, white_balance=(1.0, 1.0, 1.0), method="malvar", lut=LINEAR,
             real=False):
    """s [H, W] integers -> [H, W, 3] uint8 (real: float64, the linear tone 255 d / 65535)"""
    H, W = s.shape
    white = 2 ** bits - 1 if white_level is None else white_level
    ry, rx = divmod(PATTERNS[pattern], 2)
    y, x = np.mgrid[0:H, 0:W]
    red, blue = (y % 2 == ry) & (x % 2 == rx), (y % 2 != ry) & (x % 2 != rx)
    green, red_row = ~red & ~blue, np.broadcast_to(y % 2 == ry, (H, W))
    colour = np.where(red, 0, np.where(blue, 2, 1))
    level = np.maximum(np.minimum(s.astype(np.int64), white) - black_level, 0)
    if real:
        v = np.minimum(65535.0, level * (np.asarray(white_balance, np.float64)[colour] * 65535.0 / (white - black_level)))
    else:
        v = np.minimum(65535, (level * np.asarray(multipliers(black_level, white, white_balance), np.int64)[colour] + 2 ** 15) >> 16)
    p = v[fold(np.arange(-2, H + 2), H)][:, fold(np.arange(-2, W + 2), W)]

    def at(dy, dx):
        return p[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]

    C, H1, V1, H2, V2 = at(0, 0), at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0), at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
    D = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    if method == "malvar":
        sums = [(8 * C + 4 * (H1 + V1) - 2 * (H2 + V2), 16), (10 * C + 8 * H1 - 2 * H2 + V2 - 2 * D, 16),
                (10 * C + 8 * V1 - 2 * V2 + H2 - 2 * D, 16), (12 * C + 4 * D - 3 * (H2 + V2), 16)]
    else:
        sums = [(H1 + V1, 4), (H1, 2), (V1, 2), (D, 4)]
    if real:
        cross, along, across, diag = [np.clip(t / n, 0.0, 65535.0) for t, n in sums]
    else:
        cross, along, across, diag = [np.clip((t + n // 2) // n, 0, 65535) for t, n in sums]   # (// floors: the arithmetic >>)
    R = np.where(red, C, np.where(blue, diag, np.where(red_row, along, across)))
    G = np.where(green, C, cross)
    B = np.where(blue, C, np.where(red, diag, np.where(red_row, across, along)))
    d = np.stack([R, G, B], axis=-1)
    return d * (255.0 / 65535.0) if real else lut[d >> 4]
