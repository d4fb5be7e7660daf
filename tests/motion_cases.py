"""Inputs of the camera-motion tests: smooth random textures, panned views of one scene, and the jerky-pan sequence of
six boxes fixed in the scene."""
import functools

import numpy as np

PANS = [(0, 0), (0, 0), (0, 0), (13, 0), (-14, 5), (12, -6), (0, 0), (-13, 0), (14, 7), (-12, -7)]   # (dx, dy) per frame
PAN_HW = (192, 256)
MARGIN = 64


def _blur(a, s):
    """box filter of width s along both axes (edge-padded), float64"""
    for axis in (0, 1):
        pad = [(0, 0)] * a.ndim
        pad[axis] = (s // 2, s - 1 - s // 2)
        c = np.cumsum(np.pad(a, pad, mode="edge"), axis=axis)
        c = np.concatenate((np.zeros_like(np.take(c, [0], axis=axis)), c), axis=axis)
        n = a.shape[axis]
        a = (np.take(c, np.arange(s, s + n), axis=axis) - np.take(c, np.arange(n), axis=axis)) / s
    return a


def texture(seed, H, W, scale):
    """[H, W, 3] uint8: random values on a grid of `scale` pixels, smoothed, stretched to the whole range"""
    rng = np.random.default_rng(seed)
    h, w = -(-H // scale) + 1, -(-W // scale) + 1
    a = np.kron(rng.random((h, w, 3)), np.ones((scale, scale, 1)))[:H, :W]
    a = _blur(_blur(a, scale), scale)
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(a * 255).astype(np.uint8)


def noisy(img, seed, amp=3):
    rng = np.random.default_rng(seed)
    return np.clip(img.astype(np.int64) + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def view(canvas, hw, shift, margin=MARGIN):
    """the H x W view of a camera whose image content sits `shift` = (x, y) pixels from where the unshifted view has it"""
    H, W = hw
    y0, x0 = margin - shift[1], margin - shift[0]
    return canvas[y0:y0 + H, x0:x0 + W].copy()


def cumulative(pans):
    out, x, y = [], 0, 0
    for dx, dy in pans:
        x, y = x + dx, y + dy
        out.append((x, y))
    return out


@functools.lru_cache(maxsize=None)
def pan_frames():
    """the ten 192 x 256 frames of the jerky pan (read-only)"""
    H, W = PAN_HW
    canvas = texture(7, H + 2 * MARGIN, W + 2 * MARGIN, 12)
    frames = [view(canvas, PAN_HW, s) for s in cumulative(PANS)]
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


BOX_ORIGINS = [(40, 30), (110, 30), (180, 30), (40, 120), (110, 120), (180, 120)]   # (x1, y1) of six 12 x 24 boxes


def pan_boxes():
    """[10, 6, 4] float32 boxes fixed in the scene, scores [10, 6], labels [10, 6], count [10]"""
    boxes = np.array([[[x + sx, y + sy, x + sx + 12, y + sy + 24] for x, y in BOX_ORIGINS] for sx, sy in cumulative(PANS)],
                     np.float32)
    return boxes, np.full((10, 6), 0.9, np.float32), np.zeros((10, 6), np.int64), np.full(10, 6, np.int32)


# (H, W), the scale of the texture in pixels, the foreground rectangle (y0, x0, h, w): a quarter of the frame
RECOVER = {
    "k1": ((97, 131), 6, (40, 60, 48, 65)),
    "k2": ((192, 256), 12, (0, 0, 96, 128)),
    "k3": ((100, 333), 18, (0, 0, 100, 83)),   # one row of five blocks: the quarter is a full-height strip over two
}


@functools.lru_cache(maxsize=None)
def recover_frames(name, pans, fg_step=(-5, 4)):
    """frames of the scene panned by `pans` (cumulative, (dx, dy) per frame, frame 0 included) under +-3 of noise, with a
    textured foreground rectangle that moves by `fg_step` per frame whatever the camera does"""
    hw, scale, (y0, x0, h, w) = RECOVER[name]
    canvas = texture(11, hw[0] + 2 * MARGIN, hw[1] + 2 * MARGIN, scale)
    fg = texture(12, h + 2 * MARGIN, w + 2 * MARGIN, scale)
    out = []
    for f, s in enumerate(cumulative(pans)):
        img = view(canvas, hw, s)
        fy, fx = y0 + f * fg_step[1], x0 + f * fg_step[0]
        ys, xs = slice(max(fy, 0), min(fy + h, hw[0])), slice(max(fx, 0), min(fx + w, hw[1]))
        img[ys, xs] = fg[MARGIN + ys.start - fy:MARGIN + ys.stop - fy, MARGIN + xs.start - fx:MARGIN + xs.stop - fx]
        img = noisy(img, 100 + f)
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


def recover_pans(name, search=8, grid=160):
    """integer pans of whole cells and of odd pixels, up to the reach search * k on either axis"""
    H, W = RECOVER[name][0]
    k = max(1, -(-max(H, W) // grid))
    r = search * k
    return ((0, 0), (r, 0), (-r, r), (3, -r), (-(r - 1), 5), (k, -2 * k), (0, 0), (-7, r - 2))
