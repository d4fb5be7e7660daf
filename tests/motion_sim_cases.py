"""Inputs of the similarity camera-motion tests: views of one textured scene under a camera that zooms, rolls and pans
(a bilinear warp of motion_cases.texture canvases about the view centre), with the true (a, b) of every step, and the
sequence of eight small boxes fixed in the scene.

Convention: T_f maps the scene (the coordinates of the unmoved view) to frame f, T_f(p) = c + M_f (p - c) + t_f with c the
view centre; a step (s, theta, pan) composes as T_f(p) = c + S (T_{f-1}(p) - c) + pan, S = s [[cos, -sin], [sin, cos]], so
between frames f - 1 and f the truth is a = s cos(theta), b = s sin(theta) in the sense of include/codetr_motion.h."""
import functools
import math

import numpy as np

import motion_cases

MARGIN = 64

# (zoom, roll in rad, (pan x, pan y)) per frame, frame 0 first: zooms of 0.94 .. 1.07, rolls of up to 0.06 rad, pans of a
# few pixels; the cumulative zoom stays within 0.99 .. 1.07 and the cumulative roll within +-0.03 rad
STEPS = ((1.0, 0.0, (0, 0)), (1.05, 0.0, (2, -1)), (0.95, 0.04, (-3, 2)), (1.0, -0.06, (0, 3)), (1.07, 0.02, (1, 1)),
         (0.94, -0.03, (-2, -2)), (1.03, 0.05, (3, 0)), (0.97, -0.05, (-1, 2)), (1.04, 0.06, (2, -3)), (0.96, 0.0, (0, 0)))
PURE_PANS = ((1.0, 0.0, (0, 0)), (1.0, 0.0, (6, 0)), (1.0, 0.0, (-5, 3)), (1.0, 0.0, (2, -7)))

# name -> ((H, W), the scale of the texture in pixels, the foreground rectangle (y0, x0, h, w): a quarter of the frame)
SIZES = {
    "k1": ((97, 131), 6, (40, 60, 48, 65)),
    "k2": ((192, 256), 12, (0, 0, 96, 128)),
    "sq": ((320, 320), 12, (150, 20, 160, 160)),      # 81 blocks
    "row": ((100, 333), 18, None),                    # k = 3: one row of five collinear blocks
}


def truth(step):
    s, th, _ = step
    return s * math.cos(th), s * math.sin(th)


def cumulative(steps):
    """[(M [2, 2], t [2])] float64 per frame"""
    out, M, t = [], np.eye(2), np.zeros(2)
    for s, th, pan in steps:
        S = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        M, t = S @ M, S @ t + np.array(pan, np.float64)
        out.append((M, t))
    return out


def warp(canvas, hw, M, t, margin=MARGIN):
    """the H x W view of frame T(p) = c + M (p - c) + t of a canvas whose unmoved view starts at (margin, margin):
    bilinear, rounded to uint8; every sample lies inside the canvas (asserted)"""
    H, W = hw
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    ys, xs = np.mgrid[0:H, 0:W]
    q = np.stack((xs, ys), -1).astype(np.float64) - c - t
    p = q @ np.linalg.inv(M).T + c + margin
    x, y = p[..., 0], p[..., 1]
    assert x.min() >= 0 and y.min() >= 0 and x.max() <= canvas.shape[1] - 1 and y.max() <= canvas.shape[0] - 1
    x0 = np.minimum(np.floor(x).astype(np.int64), canvas.shape[1] - 2)
    y0 = np.minimum(np.floor(y).astype(np.int64), canvas.shape[0] - 2)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    cv = canvas.astype(np.float64)
    out = (cv[y0, x0] * (1 - fx) + cv[y0, x0 + 1] * fx) * (1 - fy) + (cv[y0 + 1, x0] * (1 - fx) + cv[y0 + 1, x0 + 1] * fx) * fy
    return np.round(out).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frames(name, steps=STEPS, foreground=False, fg_step=(-5, 4)):
    """the frames of the scene `name` under `steps` with +-3 of noise (read-only); foreground: a textured rectangle over a
    quarter of the frame that moves by fg_step per frame whatever the camera does"""
    hw, scale, rect = SIZES[name]
    canvas = motion_cases.texture(11, hw[0] + 2 * MARGIN, hw[1] + 2 * MARGIN, scale)
    out = []
    for f, (M, t) in enumerate(cumulative(steps)):
        img = warp(canvas, hw, M, t)
        if foreground:
            y0, x0, h, w = rect
            fg = motion_cases.texture(12, h + 2 * MARGIN, w + 2 * MARGIN, scale)
            fy, fx = y0 + f * fg_step[1], x0 + f * fg_step[0]
            ys, xs = slice(max(fy, 0), min(fy + h, hw[0])), slice(max(fx, 0), min(fx + w, hw[1]))
            img[ys, xs] = fg[MARGIN + ys.start - fy:MARGIN + ys.stop - fy, MARGIN + xs.start - fx:MARGIN + xs.stop - fx]
        img = motion_cases.noisy(img, 100 + f)
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


# the eight-box sequence: ten frames of 320 x 320 under STEPS, eight 8 x 12 boxes fixed in the scene
BOX_HW = SIZES["sq"][0]
BOX_CENTRES = ((60, 50), (160, 40), (260, 60), (50, 160), (270, 170), (70, 270), (160, 280), (250, 260))


@functools.lru_cache(maxsize=None)
def box_frames():
    return frames("sq")


def scene_boxes():
    """[10, 8, 4] float32 boxes (their centres moved by T_f, their sizes by the cumulative zoom), scores [10, 8], labels
    [10, 8], count [10]"""
    H, W = BOX_HW
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    boxes = []
    for M, t in cumulative(STEPS):
        z = math.sqrt(abs(np.linalg.det(M)))
        row = []
        for centre in BOX_CENTRES:
            x, y = c + M @ (np.array(centre, np.float64) - c) + t
            row.append([x - 4 * z, y - 6 * z, x + 4 * z, y + 6 * z])
        boxes.append(row)
    boxes = np.array(boxes, np.float32)
    return boxes, np.full((10, 8), 0.9, np.float32), np.zeros((10, 8), np.int64), np.full(10, 8, np.int32)
