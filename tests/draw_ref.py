"""CPU reference of the detection drawing (helper code for tests/test_draw_*.py, not collected by pytest).

Restates, in numpy with integer pixel arithmetic, the rendering include/codetr_hip.h gives for
codetr_draw_detections_*: the drawn set (score > score_thr in fp32, label in [0, C), finite coordinates, each clamped
to [-16384, 16383] and rounded as floor(x + 0.5) in fp32, x2i >= x1i and y2i >= y1i), layer 1 -- for j ascending the
edge band [x1i - a, x2i + a] x [y1i - a, y2i + a] minus the inner rectangle [x1i + b + 1, x2i - b - 1] x
[y1i + b + 1, y2i - b - 1], a = lw // 2, b = (lw - 1) // 2, blended with the class colour -- and layer 2, after every
edge, for j ascending: "<name>: <percent>" in the library's 5x7 font on a grid of 6 * len + 1 by 9 font pixels of
s x s image pixels at (x1i + lw, y1i + lw), ink opaque in the text colour, the rest blended with black.
blend(p, c) = (p * (256 - A) + c * A + 128) >> 8, A = int(alpha * 256 + 0.5) in fp32.  Clipped, never shifted.
The font is an argument: the tests pass the table the library's host-only accessor returns.
"""
import numpy as np

F = np.float32
DEFAULTS = dict(line_width=3, alpha=0.8, score_thr=0.3, text_color=(200, 200, 200), font_scale=1, draw_labels=True)
NAME_ROW = 24


def style(**kw):
    out = dict(DEFAULTS)
    assert not set(kw) - set(out), kw
    out.update(kw)
    return out


def alpha_weight(alpha):
    return int(F(alpha) * F(256.0) + F(0.5))


def blend(p, c, A):
    return (p * (256 - A) + c * A + 128) >> 8


def pixel_coord(v):
    v = np.minimum(np.maximum(F(v), F(-16384.0)), F(16383.0))
    return int(np.floor(v + F(0.5)))


def score_tenths(s):
    m = F(s) * F(1000.0)          # one rounding
    v = m + F(0.5)                # and another: never an fma
    return 0 if not v > 0 else 1000 if v >= 1000 else int(v)


def score_text(s):
    n = score_tenths(s)
    return f"{n // 10}.{n % 10}"


def names_table(classes):
    """list of str -> [C, 24] uint8: the length (<= 23), then the characters; non-ASCII-printable ones become '?'"""
    out = np.zeros((len(classes), NAME_ROW), np.uint8)
    for i, name in enumerate(classes):
        text = "".join(ch if 32 <= ord(ch) <= 126 else "?" for ch in str(name))[:NAME_ROW - 1]
        out[i, 0] = len(text)
        out[i, 1:1 + len(text)] = np.frombuffer(text.encode("ascii"), np.uint8)
    return out


def class_name(names, label):
    row = np.asarray(names)[label]
    return bytes(row[1:1 + min(int(row[0]), NAME_ROW - 1)]).decode("ascii")


def drawn_rows(boxes, scores, labels, C, score_thr):
    """-> [(j, x1i, y1i, x2i, y2i)] of the rows that are drawn, j ascending"""
    out = []
    for j in range(len(scores)):
        if not F(scores[j]) > F(score_thr) or not 0 <= int(labels[j]) < C:
            continue
        b = np.asarray(boxes[j], F)
        if not np.isfinite(b).all():
            continue
        x1, y1, x2, y2 = (pixel_coord(v) for v in b)
        if x2 >= x1 and y2 >= y1:
            out.append((j, x1, y1, x2, y2))
    return out


def edge_mask(H, W, x1, y1, x2, y2, lw):
    """bool [H, W]: the pixels of one box's edge band"""
    a, b = lw // 2, (lw - 1) // 2
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    outer = (xs >= x1 - a) & (xs <= x2 + a) & (ys >= y1 - a) & (ys <= y2 + a)
    inner = (xs >= x1 + b + 1) & (xs <= x2 - b - 1) & (ys >= y1 + b + 1) & (ys <= y2 - b - 1)
    return outer & ~inner


def text_grid(text, font):
    """bool [9, 6 * len + 1]: the font pixels that carry ink"""
    font = np.frombuffer(bytes(font), np.uint8).reshape(95, 7)
    grid = np.zeros((9, 6 * len(text) + 1), bool)
    for k, ch in enumerate(text):
        rows = font[ord(ch) - 32]
        for r in range(7):
            for c in range(5):
                grid[1 + r, 1 + 6 * k + c] = bool((rows[r] >> (4 - c)) & 1)
    return grid


def _edges_fast(img, x1, y1, x2, y2, lw, c, A):
    H, W = img.shape[:2]
    a = lw // 2
    xa, xb, ya, yb = max(x1 - a, 0), min(x2 + a, W - 1), max(y1 - a, 0), min(y2 + a, H - 1)
    if xa > xb or ya > yb:
        return
    m = edge_mask(H, W, x1, y1, x2, y2, lw)[ya:yb + 1, xa:xb + 1]
    region = img[ya:yb + 1, xa:xb + 1]
    region[m] = blend(region[m], np.asarray(c, np.int32)[None, :], A)


def draw(image, boxes, scores, labels, names, palette, font, st=None):
    """one image [H, W, 3] uint8 and its detections (fp32 values of the storage type) -> the drawn image (a copy)"""
    st = style(**(st or {}))
    names = names_table(names) if isinstance(names, (list, tuple)) else np.asarray(names)
    palette = np.asarray(palette, np.int32).reshape(-1, 3)
    C, lw, A = len(palette), int(st["line_width"]), alpha_weight(st["alpha"])
    img = np.asarray(image).astype(np.int32)
    H, W = img.shape[:2]
    rows = drawn_rows(boxes, scores, labels, C, st["score_thr"])
    for j, x1, y1, x2, y2 in rows:
        _edges_fast(img, x1, y1, x2, y2, lw, palette[int(labels[j])], A)
    if st["draw_labels"]:
        tc = np.asarray(st["text_color"], np.int32)
        for j, x1, y1, x2, y2 in rows:
            text = class_name(names, int(labels[j])) + ": " + score_text(scores[j])
            s = int(st["font_scale"]) * (2 if (x2 - x1) * (y2 - y1) >= 15400 else 1)
            ink = np.repeat(np.repeat(text_grid(text, font), s, 0), s, 1)
            ox, oy = x1 + lw, y1 + lw
            xa, xb, ya, yb = max(ox, 0), min(ox + ink.shape[1], W), max(oy, 0), min(oy + ink.shape[0], H)
            if xa >= xb or ya >= yb:
                continue
            ink = ink[ya - oy:yb - oy, xa - ox:xb - ox]
            region = img[ya:yb, xa:xb]
            region[...] = np.where(ink[:, :, None], tc[None, None, :], blend(region, 0, A))
    return img.astype(np.uint8)


def draw_buffer(buf, rows, boxes, scores, labels, count, names, palette, font, st=None):
    """the whole launch: flat uint8 `buf` with image n [H, W, 3] at rows[n] = (offset, H, W); boxes [N, Q, 4], scores
    [N, Q], labels [N, Q], count [N] -> the drawn buffer (a copy; bytes outside the images unchanged)"""
    out = np.array(buf, np.uint8, copy=True)
    for n, (off, H, W) in enumerate(rows):
        c = min(max(int(count[n]), 0), len(scores[n]))
        img = out[off:off + H * W * 3].reshape(H, W, 3)
        out[off:off + H * W * 3] = draw(img, boxes[n][:c], scores[n][:c], labels[n][:c], names, palette, font,
                                        st).reshape(-1)
    return out
