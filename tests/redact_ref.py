"""The redaction rule of include/codetr_redact.h restated in numpy, operation by operation: integers, and fp32 with one
rounding per operation.  The kernel (csrc/redact.hip) is compared with it byte for byte, no tolerance.

"blur" is the library's own (a box filter over fixed cells and a tent reconstruction); parity with OpenCV's blur is
unpinned: cv2 is not installed here.
"""
import numpy as np

F = np.float32
DEFAULTS = dict(mode="pixelate", score_thr=0.3, expand=0.1, shape="box", cell=16, fill=(0, 0, 0))
LO, HI = F(-16384.0), F(16383.0)


def settings(**kw):
    st = dict(DEFAULTS)
    assert not set(kw) - set(st), kw
    st.update(kw)
    return st


def selected_rows(boxes, scores, labels, count, score_thr, select=None):
    """the rows a call redacts ("Selection"): boxes [Q, 4], scores [Q] float32 (the stored values widened), labels [Q],
    count; select: a sequence of C flags or None -> [j]"""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    Q = len(boxes)
    cnt = min(max(int(count), 0), Q)
    out = []
    for j in range(cnt):
        if not F(scores[j]) > F(score_thr):          # strict; a NaN fails
            continue
        label = int(labels[j])
        if select is not None and not (0 <= label < len(select) and select[label] != 0):
            continue
        if not np.isfinite(boxes[j]).all():
            continue
        out.append(j)
    return out


def _clamp(v):
    return np.minimum(np.maximum(F(v), LO), HI)


def region(box, expand):
    """(X1, Y1, X2, Y2) of a redacted row, or None when the region does not exist"""
    x1, y1, x2, y2 = (_clamp(v) for v in box)
    e = F(expand)
    w, h = F(x2 - x1), F(y2 - y1)
    ex, ey = F(e * w), F(e * h)
    a1, a2 = _clamp(F(x1 - ex)), _clamp(F(x2 + ex))
    b1, b2 = _clamp(F(y1 - ey)), _clamp(F(y2 + ey))
    X1, X2 = int(np.floor(a1)), int(np.ceil(a2)) - 1
    Y1, Y2 = int(np.floor(b1)), int(np.ceil(b2)) - 1
    return (X1, Y1, X2, Y2) if X2 >= X1 and Y2 >= Y1 else None


def region_mask(H, W, reg, shape):
    """the pixels of one region inside an H x W image -> bool [H, W]"""
    X1, Y1, X2, Y2 = reg
    m = np.zeros((H, W), bool)
    xa, xb, ya, yb = max(X1, 0), min(X2, W - 1), max(Y1, 0), min(Y2, H - 1)
    if xa > xb or ya > yb:
        return m
    if shape == "box":
        m[ya:yb + 1, xa:xb + 1] = True
        return m
    Ww, Hh = X2 - X1 + 1, Y2 - Y1 + 1
    x = np.arange(xa, xb + 1, dtype=np.int64)[None, :]
    y = np.arange(ya, yb + 1, dtype=np.int64)[:, None]
    m[ya:yb + 1, xa:xb + 1] = ((2 * x + 1 - X1 - X2 - 1) * Hh) ** 2 + ((2 * y + 1 - Y1 - Y2 - 1) * Ww) ** 2 <= (Ww * Hh) ** 2
    return m


def mask(H, W, boxes, scores, labels, count, st, select=None):
    """the masked pixels of one image -> (bool [H, W], the redacted rows)"""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    rows = selected_rows(boxes, scores, labels, count, st["score_thr"], select)
    m = np.zeros((H, W), bool)
    for j in rows:
        reg = region(boxes[j], st["expand"])
        if reg is not None:
            m |= region_mask(H, W, reg, st["shape"])
    return m, rows


def cell_means(image, cell):
    """[ceil(H / cell), ceil(W / cell), 3] int64: (sum + n / 2) / n per clipped cell and channel"""
    H, W = image.shape[:2]
    gh, gw = -(-H // cell), -(-W // cell)
    out = np.zeros((gh, gw, 3), np.int64)
    for k in range(gh):
        for i in range(gw):
            block = image[k * cell:(k + 1) * cell, i * cell:(i + 1) * cell].astype(np.int64).reshape(-1, 3)
            n = len(block)
            out[k, i] = (block.sum(0) + n // 2) // n
    return out


def _tent(size, cell, cells):
    """per pixel coordinate: (index 0, index 1, weight 0, weight 1), the indices clamped to the grid"""
    c = cell
    u = 2 * np.arange(size, dtype=np.int64) + 1 - c
    i0 = u // (2 * c)                       # floor
    f = u - 2 * c * i0
    return np.clip(i0, 0, cells - 1), np.clip(i0 + 1, 0, cells - 1), 2 * c - f, f


def blurred(image, cell):
    """the value "blur" gives every pixel, were it masked -> uint8 [H, W, 3]"""
    H, W = image.shape[:2]
    means = cell_means(image, cell)
    gh, gw = means.shape[:2]
    x0, x1, wx0, wx1 = _tent(W, cell, gw)
    y0, y1, wy0, wy1 = _tent(H, cell, gh)
    lc = cell.bit_length() - 1
    total = ((wy0[:, None] * wx0[None, :])[..., None] * means[y0][:, x0] + (wy0[:, None] * wx1[None, :])[..., None] * means[y0][:, x1]
             + (wy1[:, None] * wx0[None, :])[..., None] * means[y1][:, x0] + (wy1[:, None] * wx1[None, :])[..., None] * means[y1][:, x1])
    return ((total + 2 * cell * cell) >> (2 * lc + 2)).astype(np.uint8)


def pixelated(image, cell):
    """the value "pixelate" gives every pixel, were it masked -> uint8 [H, W, 3]"""
    H, W = image.shape[:2]
    means = cell_means(image, cell)
    return means[np.arange(H) // cell][:, np.arange(W) // cell].astype(np.uint8)


def redact(image, boxes, scores, labels, st=None, select=None, count=None):
    """one image [H, W, 3] uint8 -> (the redacted copy, the redacted rows); count None = every row"""
    st = settings(**(st or {}))
    image = np.asarray(image, np.uint8)
    H, W = image.shape[:2]
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    m, rows = mask(H, W, boxes, scores, labels, len(boxes) if count is None else count, st, select)
    out = image.copy()
    if not m.any():
        return out, rows
    if st["mode"] == "fill":
        out[m] = np.asarray(st["fill"], np.uint8)
    elif st["mode"] == "pixelate":
        out[m] = pixelated(image, st["cell"])[m]
    else:
        assert st["mode"] == "blur"
        out[m] = blurred(image, st["cell"])[m]
    return out, rows


def redact_buffer(buf, rows, boxes, scores, labels, count, st=None, select=None):
    """the images `rows` [(offset, H, W)] of a flat uint8 buffer, boxes [N, Q, 4], scores / labels [N, Q], count [N]
    -> the redacted copy of the buffer"""
    out = np.asarray(buf, np.uint8).copy()
    for n, (off, H, W) in enumerate(rows):
        img = buf[off:off + H * W * 3].reshape(H, W, 3)
        out[off:off + H * W * 3] = redact(img, boxes[n], scores[n], labels[n], st, select, count[n])[0].reshape(-1)
    return out
