"""The sequences and geometry cases of the appearance tests (include/codetr_appearance.h).

Sequences: 120 x 160 RGB frames, background noise in [100, 140), objects of a solid colour +- 6 of noise filling their
16 x 32 boxes, every label 0, every score 0.9.  `sequence(name)` -> (frames [F, 120, 160, 3] uint8, dets: per frame a list
of (x1, y1, x2, y2) in row order, names: per frame the objects present).  The row order is the order of OBJECTS[name].

  reentry  green fixed at (100, 20); red at (10 + 3 f, 30) for f < 6, absent for 6 <= f < 14, then at (10 + 3 f + 4, 58):
           it returns 28 px below its constant-velocity prediction, where the overlap is 0.
  lanes    green fixed at (130, 10); red at (10 + 3 f, 20) and blue at (10 + 3 f, 62) for f < 8, both absent for
           8 <= f < 16, then red at (10 + 3 f + 3, 60) and blue at (10 + 3 f - 2, 22): each comes out nearer to the
           other's prediction.
"""
import numpy as np

H, W, BW, BH = 120, 160, 16, 32
COLOURS = dict(red=(200, 40, 40), green=(40, 200, 40), blue=(40, 40, 200))
OBJECTS = dict(reentry=("green", "red"), lanes=("green", "red", "blue"))
FRAMES = dict(reentry=24, lanes=24)


def position(name, obj, f):
    """the top-left corner of `obj` in frame f of sequence `name`, or None while it is hidden"""
    if name == "reentry":
        if obj == "green":
            return 100, 20
        if f < 6:
            return 10 + 3 * f, 30
        return None if f < 14 else (10 + 3 * f + 4, 58)
    if obj == "green":
        return 130, 10
    if 8 <= f < 16:
        return None
    if obj == "red":
        return (10 + 3 * f, 20) if f < 8 else (10 + 3 * f + 3, 60)
    return (10 + 3 * f, 62) if f < 8 else (10 + 3 * f - 2, 22)


def sequence(name, seed=0):
    rng = np.random.default_rng(seed)
    frames, dets, names = [], [], []
    for f in range(FRAMES[name]):
        img = rng.integers(100, 140, (H, W, 3), dtype=np.int64)
        boxes, present = [], []
        for obj in OBJECTS[name]:
            p = position(name, obj, f)
            if p is None:
                continue
            x, y = p
            noise = rng.integers(-6, 7, (BH, BW, 3), dtype=np.int64)
            img[y:y + BH, x:x + BW] = np.array(COLOURS[obj], np.int64) + noise
            boxes.append((float(x), float(y), float(x + BW), float(y + BH)))
            present.append(obj)
        frames.append(img.astype(np.uint8))
        dets.append(boxes)
        names.append(present)
    return np.stack(frames), dets, names


def geometry_boxes(Hh, Ww):
    """boxes against an Hh x Ww image: inside, over each edge, wholly outside, larger than the image, x2 == W, 1 x 1,
    0.25 wide, w <= 0, NaN, inf (1e30 is added by the f32 test alone: it is inf in f16)"""
    nan, inf = float("nan"), float("inf")
    return [
        (5.0, 4.0, 21.0, 30.0),                    # inside
        (-7.0, 6.0, 9.0, 20.0),                    # over the left edge
        (Ww - 9.0, 3.0, Ww + 8.0, 17.0),           # over the right edge
        (10.0, -11.0, 26.0, 9.0),                  # over the top edge
        (12.0, Hh - 6.0, 30.0, Hh + 13.0),         # over the bottom edge
        (-60.0, -50.0, -20.0, -10.0),              # wholly outside (above, left)
        (Ww + 10.0, Hh + 5.0, Ww + 40.0, Hh + 45.0),   # wholly outside (below, right)
        (-20.0, -30.0, Ww + 25.0, Hh + 35.0),      # larger than the image
        (Ww - 12.0, 2.0, float(Ww), 12.0),         # x2 == W
        (7.0, 9.0, 8.0, 10.0),                     # 1 x 1
        (13.5, 5.0, 13.75, 25.0),                  # 0.25 wide
        (20.0, 5.0, 20.0, 25.0),                   # w == 0
        (22.0, 5.0, 18.0, 25.0),                   # w < 0
        (4.0, 25.0, 14.0, 20.0),                   # h < 0
        (nan, 5.0, 20.0, 25.0),
        (3.0, 5.0, inf, 25.0),
        (3.0, -inf, 20.0, 25.0),
        (2.25, 3.5, 30.75, 33.25),                 # fractional corners
    ]


def edge_image(Hh, Ww, seed):
    """an image whose channels take the values on both sides of every bin edge (63 / 64, 127 / 128, 191 / 192) and 0 / 255"""
    rng = np.random.default_rng(seed)
    values = np.array([0, 63, 64, 127, 128, 191, 192, 255], np.uint8)
    return values[rng.integers(0, len(values), (Hh, Ww, 3))]
