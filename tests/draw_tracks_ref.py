"""CPU reference of the track drawing (helper code for tests/test_draw_tracks_*.py, not collected by pytest).

Restates include/codetr_draw_tracks.h in numpy: the trail state and its per-row update (`Trails`), the integer capsule
test (`covers`, `trail_mask`) and the three layers (`draw`): trails blended once per trail and pixel, outlines in the
id's colour, labels with "#<id> " in front.  The outline and label rules are tests/draw_ref.py's.
"""
import numpy as np

import draw_ref as D

F = np.float32
DEFAULTS = dict(color_by="track", show_id=True, trail=30, trail_width=2, trail_alpha=0.6, anchor="center", tentative=False,
                untracked=True, retain=30)


def covers(x, y, p0, p1, w):
    """is pixel (x, y) covered by the capsule of p0 -> p1?  Python ints or int64 arrays (the header's bound: no overflow)"""
    dx, dy, ex, ey = p1[0] - p0[0], p1[1] - p0[1], x - p0[0], y - p0[1]
    L, t = dx * dx + dy * dy, ex * dx + ey * dy
    gx, gy, cross = x - p1[0], y - p1[1], ex * dy - ey * dx
    first, last = ex * ex + ey * ey <= w * w // 4, gx * gx + gy * gy <= w * w // 4
    return np.where((L == 0) | (t <= 0), first, np.where(t >= L, last, cross * cross <= (w * w * L) // 4))


def trail_mask(H, W, points, w):
    """bool [H, W]: the union of the capsules of a polyline; one point is a disc"""
    ys, xs = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    pts = [tuple(int(v) for v in p) for p in points]
    m = np.zeros((H, W), bool)
    for p0, p1 in zip(pts, pts[1:] or pts):
        m |= covers(xs, ys, p0, p1, w)
    return m


class Trails:
    """one stream's trail state: T entries of K points; update() is one row of codetr_trail_update_*"""

    def __init__(self, T, K):
        self.T, self.K, self.f = T, K, 0
        self.id, self.last, self.len, self.head = (np.zeros(T, np.int32) for _ in range(4))
        self.ring = np.zeros((T, K, 2), np.int16)

    def state(self):
        return np.concatenate([np.array([self.f, 0, 0, 0], np.int32).view(np.uint8)] +
                              [a.reshape(-1).view(np.uint8) for a in (self.id, self.last, self.len, self.head, self.ring)])

    def points(self, t):
        return [self.ring[t, (self.head[t] + k) % self.K] for k in range(self.len[t])]

    def update(self, boxes, ids, count, retain=30, anchor="center", tentative=False):
        """boxes [Q, 4] fp32 values of the storage type, ids [Q] -> the row's snapshot bytes"""
        T, K, f = self.T, self.K, self.f
        for t in range(T):
            if self.id[t] != 0 and f - self.last[t] >= retain:
                self.id[t] = self.last[t] = self.len[t] = self.head[t] = 0
                self.ring[t] = 0
        seen, fresh = set(), []
        for j in range(min(max(int(count), 0), len(ids))):
            i, b = int(ids[j]), np.asarray(boxes[j], F)
            if not (i > 0 or (tentative and i != 0)) or not np.isfinite(b).all() or abs(i) in seen:
                continue
            seen.add(abs(i))
            ya = b[3] if anchor == "bottom" else (b[1] + b[3]) * F(0.5)
            pt = (D.pixel_coord((b[0] + b[2]) * F(0.5)), D.pixel_coord(ya))
            hit = np.flatnonzero(self.id == abs(i))
            if len(hit) == 0:
                fresh.append((abs(i), pt))
                continue
            t = hit[0]
            if self.len[t] < K:
                self.ring[t, (self.head[t] + self.len[t]) % K] = pt
                self.len[t] += 1
            else:
                self.ring[t, self.head[t]] = pt
                self.head[t] = (self.head[t] + 1) % K
            self.last[t] = f
        for (key, pt), t in zip(fresh, np.flatnonzero(self.id == 0)):   # ascending j takes ascending free entry
            self.id[t], self.last[t], self.len[t], self.head[t], self.ring[t, 0] = key, f, 1, 0, pt
        self.f += 1
        box, pts = np.zeros((T, 4), np.int16), np.zeros((T, K, 2), np.int16)
        for t in range(T):
            if self.len[t]:
                p = np.array(self.points(t))
                pts[t, :len(p)], box[t] = p, (*p.min(0), *p.max(0))
        return np.concatenate([a.reshape(-1).view(np.uint8) for a in (self.id.copy(), self.len.copy(), box, pts)])


def snapshot_trails(snap, T, K):
    """a snapshot's bytes -> [(id, points [len, 2])] of its live entries, entry order"""
    snap = np.ascontiguousarray(snap)
    ids, lens = snap[:4 * T].view(np.int32), snap[4 * T:8 * T].view(np.int32)
    pts = snap[16 * T:].view(np.int16).reshape(T, K, 2)
    return [(int(ids[t]), pts[t, :lens[t]]) for t in range(T) if ids[t] != 0 and lens[t] >= 1]


def draw(image, boxes, scores, labels, ids, trails, names, palette, track_palette, font, st=None):
    """one image [H, W, 3] uint8, its detections with their ids [Q] and its trails [(id, points)] -> the drawn copy"""
    st = {**D.DEFAULTS, **DEFAULTS, **(st or {})}
    names = D.names_table(names) if isinstance(names, (list, tuple)) else np.asarray(names)
    palette, tp = np.asarray(palette, np.int32).reshape(-1, 3), np.asarray(track_palette, np.int32).reshape(-1, 3)
    lw, A, At = int(st["line_width"]), D.alpha_weight(st["alpha"]), D.alpha_weight(st["trail_alpha"])
    img = np.asarray(image).astype(np.int32)
    H, W = img.shape[:2]
    for i, pts in trails:
        m = trail_mask(H, W, pts, int(st["trail_width"]))
        img[m] = D.blend(img[m], tp[(i - 1) % len(tp)][None, :], At)
    rows = [r for r in D.drawn_rows(boxes, scores, labels, len(palette), st["score_thr"]) if ids[r[0]] != 0 or st["untracked"]]
    for j, x1, y1, x2, y2 in rows:
        i = abs(int(ids[j]))
        c = tp[(i - 1) % len(tp)] if st["color_by"] == "track" and i else palette[int(labels[j])]
        D._edges_fast(img, x1, y1, x2, y2, lw, c, A)
    tc = np.asarray(st["text_color"], np.int32)
    for j, x1, y1, x2, y2 in rows if st["draw_labels"] else []:
        i = int(ids[j])
        text = (f"{'~' if i < 0 else '#'}{abs(i)} " if st["show_id"] and i else "") + \
            D.class_name(names, int(labels[j])) + ": " + D.score_text(scores[j])
        s = int(st["font_scale"]) * (2 if (x2 - x1) * (y2 - y1) >= 15400 else 1)
        ink = np.repeat(np.repeat(D.text_grid(text, font), s, 0), s, 1)
        ox, oy = x1 + lw, y1 + lw
        xa, xb, ya, yb = max(ox, 0), min(ox + ink.shape[1], W), max(oy, 0), min(oy + ink.shape[0], H)
        if xa < xb and ya < yb:
            region = img[ya:yb, xa:xb]
            region[...] = np.where(ink[ya - oy:yb - oy, xa - ox:xb - ox, None], tc[None, None, :], D.blend(region, 0, A))
    return img.astype(np.uint8)


def draw_buffer(buf, rows, boxes, scores, labels, count, ids, trails, names, palette, track_palette, font, st=None):
    """the whole launch on a flat uint8 `buf` (image n at rows[n] = (offset, H, W)); trails: per image [(id, points)] ->
    the drawn buffer (a copy; bytes outside the images unchanged)"""
    out = np.array(buf, np.uint8, copy=True)
    for n, (off, H, W) in enumerate(rows):
        c = min(max(int(count[n]), 0), len(scores[n]))
        img = out[off:off + H * W * 3].reshape(H, W, 3)
        out[off:off + H * W * 3] = draw(img, boxes[n][:c], scores[n][:c], labels[n][:c], ids[n][:c], trails[n], names,
                                        palette, track_palette, font, st).reshape(-1)
    return out
