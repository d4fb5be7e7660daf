"""The contrast-enhancement rule of include/codetr_enhance.h restated in numpy int64, step by step; with real=True steps 6
and 7 in float64 without their roundings (the real-number computation the header's bound is against)."""
import math

import numpy as np

BINS = np.arange(256)


def clip_count(clip_limit, T):
    return T if clip_limit is None else max(1, (math.floor(256 * clip_limit + 0.5) * T) >> 16)


def redistribute(h, C):
    """step 5 on histograms [..., 256]"""
    E = np.maximum(h - C, 0).sum(-1, keepdims=True)
    r = E & 255
    s = 256 // np.maximum(r, 1)
    return np.minimum(h, C) + (E >> 8) + ((r > 0) & (BINS % s == 0) & (BINS // s < r))


def _axis(n, g, t):
    """step 7 along one axis of n pixels, g tiles of t: the two tile indices and the weight of the second"""
    u = 2 * np.arange(n) + 1 - t
    j = u // (2 * t)
    return np.clip(j, 0, g - 1), np.clip(j + 1, 0, g - 1), u - 2 * t * j


def enhance(image, grid=(8, 8), clip_limit=2.0, real=False):
    """image [H, W, 3] uint8 -> the enhanced image (uint8; float64 with real=True)"""
    rgb = image.astype(np.int64)
    (H, W), (gy, gx) = rgb.shape[:2], grid
    th, tw = -(-H // gy), -(-W // gx)
    T = th * tw
    Y = (77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8
    iy, ix = np.arange(gy * th), np.arange(gx * tw)                              # step 3
    padded = Y[np.where(iy < H, iy, 2 * (H - 1) - iy)][:, np.where(ix < W, ix, 2 * (W - 1) - ix)]
    tile = (iy // th)[:, None] * gx + ix // tw
    h = np.bincount((tile * 256 + padded).ravel(), minlength=gy * gx * 256).reshape(gy, gx, 256)
    cum = np.cumsum(redistribute(h, clip_count(clip_limit, T)), -1)
    L = 255 * cum / T if real else (255 * cum + (T >> 1)) // T
    (j0, j1, wy), (i0, i1, wx) = _axis(H, gy, th), _axis(W, gx, tw)
    wy, j0, j1 = wy[:, None], j0[:, None], j1[:, None]
    S = (2 * th - wy) * ((2 * tw - wx) * L[j0, i0, Y] + wx * L[j0, i1, Y]) + wy * ((2 * tw - wx) * L[j1, i0, Y] + wx * L[j1, i1, Y])
    Yn = S / (4 * T) if real else (S + 2 * T) // (4 * T)
    out = np.clip(rgb + (Yn - Y)[..., None], 0, 255)
    return out if real else out.astype(np.uint8)
