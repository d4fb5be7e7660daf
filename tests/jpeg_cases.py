"""The images test_jpeg_gpu.py sends through the encoder, and their files from the restatement (computed once per
process).  test_jpeg_cpu.py asserts, on the restatement's counters, that this list reaches every branch of the entropy
coder -- a coverage condition of the inputs, checked where no GPU is needed.

Shapes are (W, H).  One pass of a workgroup handles CODETR_JPEG_PASS_PIXELS = 448 pixels of an MCU row (28 MCUs at
4:2:0, 56 at 4:4:4), so the 4112-wide image takes ten passes per row with a short last one; 40 x 147 has ten MCU rows at
4:2:0 and 40 x 75 ten at 4:4:4 (the RST counter wraps after eight).
"""
import functools

import numpy as np

import jpeg_ref

SHAPES = [(1, 1), (8, 8), (16, 16), (17, 9), (33, 31), (40, 147), (40, 75), (4112, 16)]
QUALITIES = (1, 50, 90, 100)
SUBSAMPLINGS = ("420", "444")


def content(kind, W, H, seed=0):
    rng = np.random.default_rng(seed + 1000 * W + H)
    if kind == "zeros":
        return np.zeros((H, W, 3), np.uint8)
    if kind == "ones":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    if kind == "gradient":
        return np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(W + H - 2, 1)],
                        -1).astype(np.uint8)
    if kind == "checker":     # alternating black and white 16 x 16 squares: DC differences of category 11 at quality 100
        return np.repeat((((xx // 16) + (yy // 16)) % 2 * 255).astype(np.uint8)[..., None], 3, -1)
    raise ValueError(kind)


# what each (quality, subsampling) group encodes: every shape with the contents listed for the quality
CONTENTS = {1: ("noise", "zeros"), 50: ("checker", "zeros", "noise"), 90: ("ones", "gradient"),
            100: ("noise", "checker", "ones")}
EXTRA = {10: ("gradient",)}     # the gradient at quality 10


def group(quality, subsampling):
    """[(name, image)] of one (quality, subsampling) group"""
    out = []
    for W, H in SHAPES:
        if (W, H) == (40, 75) and subsampling != "444" or (W, H) == (40, 147) and subsampling != "420":
            continue
        for kind in CONTENTS.get(quality, ()) + EXTRA.get(quality, ()):
            out.append((f"{kind}-{W}x{H}", content(kind, W, H)))
    return out


GROUPS = [(q, s) for q in QUALITIES + (10,) for s in SUBSAMPLINGS]


@functools.lru_cache(maxsize=None)
def expected(quality, subsampling):
    """(files, the restatement's counters summed over the group); computed once, never changed"""
    stats = jpeg_ref.new_stats()
    files = [jpeg_ref.encode(img, quality, subsampling, stats) for _, img in group(quality, subsampling)]
    return files, stats
