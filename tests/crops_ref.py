"""The object-crop rule of include/codetr_crops.h restated in numpy, operation by operation: integers (int64: ample at the
test shapes; the header gives the widths at the limits), fp32 with one rounding per operation for the region and the
tensor form.  The kernels (csrc/crops.hip) are compared with it byte for byte.  CASES is the table both test files share."""
import numpy as np

F = np.float32
DEFAULTS = dict(size=None, score_thr=0.3, expand=0.0, fit="stretch", pad_value=(114, 114, 114), max_per_img=32, tensor=None,
                download=True)
SIZES = [(70, 131), (5, 7), (64, 128)]   # (H, W) of the three test images
# (name, image, box (x1, y1, x2, y2) with expand 0, output (w, h))
CASES = [
    ("non_integer_reduction", 0, (10.0, 20.0, 63.0, 57.0), (16, 8)),
    ("enlargement", 0, (40.0, 30.0, 43.0, 35.0), (16, 8)),
    ("identity", 0, (5.0, 9.0, 21.0, 17.0), (16, 8)),
    ("one_pixel", 0, (100.0, 50.0, 101.0, 51.0), (16, 8)),
    ("clipped_left", 0, (-20.5, 10.0, 9.0, 40.0), (16, 8)),
    ("clipped_top", 0, (30.0, -7.0, 60.0, 12.5), (16, 8)),
    ("clipped_right", 0, (120.0, 10.0, 150.0, 40.0), (16, 8)),
    ("clipped_bottom", 0, (30.0, 60.0, 60.0, 99.0), (16, 8)),
    ("whole_image", 0, (0.0, 0.0, 131.0, 70.0), (8, 8)),
    ("seams_and_tails", 0, (3.0, 2.0, 128.0, 69.0), (24, 40)),
    ("tiny_image", 1, (0.0, 0.0, 7.0, 5.0), (16, 8)),
    ("largest_output", 2, (0.0, 0.0, 128.0, 64.0), (512, 512)),
    ("two_columns_per_lane", 2, (1.0, 1.0, 120.0, 60.0), (200, 9)),
]


def region(box, expand, H, W):
    """the half-open rectangle (x0, y0, x1, y1) of a row, clipped to the H x W image, or None when it is empty"""
    clamp = lambda v: np.minimum(np.maximum(F(v), F(-16384.0)), F(16383.0))  # noqa: E731
    x1, y1, x2, y2 = (clamp(v) for v in box)
    ex, ey = F(F(expand) * F(x2 - x1)), F(F(expand) * F(y2 - y1))
    X1, X2 = int(np.floor(clamp(F(x1 - ex)))), int(np.ceil(clamp(F(x2 + ex)))) - 1
    Y1, Y2 = int(np.floor(clamp(F(y1 - ey)))), int(np.ceil(clamp(F(y2 + ey)))) - 1
    x0, y0, xe, ye = max(X1, 0), max(Y1, 0), min(X2 + 1, W), min(Y2 + 1, H)
    return (x0, y0, xe, ye) if X2 >= X1 and Y2 >= Y1 and xe > x0 and ye > y0 else None


def inner_rect(fit, Rw, Rh, w, h):
    """(ox, oy, iw, ih) ("Fit")"""
    iw, ih = w, h
    if fit == "pad" and Rw * h >= Rh * w:
        ih = min(max((2 * Rh * w + Rw) // (2 * Rw), 1), h)
    elif fit == "pad":
        iw = min(max((2 * Rw * h + Rh) // (2 * Rh), 1), w)
    return (w - iw) // 2, (h - ih) // 2, iw, ih


def weights(n, R):
    """[n, R] integer weights wt(j, s) of an axis ("Resampling")"""
    j, s = np.arange(n, dtype=np.int64)[:, None], np.arange(R, dtype=np.int64)[None, :]
    return np.maximum(2 * max(n, R) - np.abs((2 * s + 1) * n - (2 * j + 1) * R), 0)


def resample(patch, iw, ih):
    """patch [Rh, Rw, 3] uint8 -> [ih, iw, 3] uint8: horizontal pass to 8.8 fixed point, vertical pass, one rounding"""
    wx, wy = weights(iw, patch.shape[1]), weights(ih, patch.shape[0])
    nx, D = wx.sum(1)[None, :, None], 256 * wy.sum(1)[:, None, None]
    t = (np.einsum("is,ysc->yic", wx, patch.astype(np.int64)) * 256 + nx // 2) // nx
    return ((np.einsum("jy,yic->jic", wy, t) + D // 2) // D).astype(np.uint8)


def crop(image, reg, st):
    """one image [H, W, 3] uint8 and a region -> the [h, w, 3] uint8 crop"""
    (w, h), (x0, y0, x1, y1) = st["size"], reg
    ox, oy, iw, ih = inner_rect(st["fit"], x1 - x0, y1 - y0, w, h)
    out = np.empty((h, w, 3), np.uint8)
    out[:] = np.asarray(st["pad_value"], np.uint8)
    out[oy:oy + ih, ox:ox + iw] = resample(image[y0:y1, x0:x1], iw, ih)
    return out


def crops(image, boxes, scores, labels, st, select=None, count=None):
    """one image -> ([k, h, w, 3] uint8, the cropped rows in order ("Selection")); count None = every row"""
    st = dict(DEFAULTS, **st)
    H, W = image.shape[:2]
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    rows = []
    for j in range(min(max(int(len(boxes) if count is None else count), 0), len(boxes))):
        label = int(labels[j])
        if len(rows) < st["max_per_img"] and F(scores[j]) >= F(st["score_thr"]) and np.isfinite(boxes[j]).all() \
                and (select is None or (0 <= label < len(select) and select[label] != 0)) \
                and region(boxes[j], st["expand"], H, W) is not None:
            rows.append(j)
    out = [crop(image, region(boxes[j], st["expand"], H, W), st) for j in rows]
    return (np.stack(out) if out else np.zeros((0, st["size"][1], st["size"][0], 3), np.uint8)), rows


def normalised(crops_u8, mean, std):
    """[k, h, w, 3] uint8 -> [k, 3, h, w] fp32: ((float)v - mean) / std, one rounding each"""
    v = crops_u8.astype(F).transpose(0, 3, 1, 2)
    return (v - np.asarray(mean, F)[None, :, None, None]) / np.asarray(std, F)[None, :, None, None]
