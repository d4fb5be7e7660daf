#!/usr/bin/env python3
"""Write tests/golden/jpeg_dec/*.jpg: the JPEG files the decoder tests read (tests/jpeg_dec_cases.py lists them).  They are
written by Pillow (libjpeg-turbo) once and committed, because the tests must also run where Pillow is absent; the
contents are seeded, so a rerun with the same Pillow reproduces them.
    python tools/gen_jpeg_dec_fixtures.py"""
import io
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_dec")
SIZES = [(1, 1), (2, 3), (3, 2), (8, 8), (16, 16), (17, 9), (33, 31), (37, 53)]   # (W, H)
SUBS = {"444": 0, "422": 1, "420": 2}
# per size, in turn: quality, optimize, restart (None, ("blocks", 3) or ("rows", 1)), content
OPTIONS = [(90, False, None, "noise"), (30, True, ("blocks", 3), "gradient"), (100, False, ("rows", 1), "blocks"),
           (90, True, None, "gradient"), (100, True, ("blocks", 3), "noise"), (30, False, ("rows", 1), "noise"),
           (90, False, ("blocks", 3), "blocks"), (100, False, None, "noise")]


def content(kind, W, H, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    if kind == "gradient":
        base = np.stack([xx * 5 + yy, yy * 7 + 30, 255 - xx * 3 - yy * 2], -1) % 256
        return np.clip(base + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    if kind == "blocks":   # 8x8 blocks that alternate between black and white: the largest DC differences
        on = ((xx // 8 + yy // 8) % 2).astype(np.uint8) * 255
        return np.repeat(on[..., None], 3, 2)
    raise ValueError(kind)


def save(im, **kw):
    f = io.BytesIO()
    im.save(f, "JPEG", **kw)
    return f.getvalue()


def files():
    out = {}
    for si, (W, H) in enumerate(SIZES):
        for bi, sub in enumerate(("444", "422", "420", "grey")):
            q, opt, rst, kind = OPTIONS[(si + bi) % len(OPTIONS)]
            arr = content(kind, W, H, 100 * si + bi)
            im = Image.fromarray(arr).convert("L") if sub == "grey" else Image.fromarray(arr)
            kw = dict(quality=q, optimize=opt)
            if sub != "grey":
                kw["subsampling"] = SUBS[sub]
            name = f"{sub}_{W}x{H}_q{q}" + ("_opt" if opt else "")
            if rst:
                kw["restart_marker_" + rst[0]] = rst[1]
                name += "_r" + rst[0][0] + str(rst[1])
            out[name] = save(im, **kw)
    out["420_5x40_q90"] = save(Image.fromarray(content("gradient", 5, 40, 900)), quality=90, subsampling=2)
    out["420_320x240_noise_q90"] = save(Image.fromarray(content("noise", 320, 240, 901)), quality=90, subsampling=2)
    out["420_320x240_gradient_q90_rr1"] = save(Image.fromarray(content("gradient", 320, 240, 902)), quality=90, subsampling=2,
                                               restart_marker_rows=1)
    out["422_320x240_gradient_q75"] = save(Image.fromarray(content("gradient", 320, 240, 903)), quality=75, subsampling=1)
    small = Image.fromarray(content("gradient", 24, 24, 904))
    out["refuse_progressive"] = save(small, quality=90, progressive=True)
    out["refuse_cmyk"] = save(small.convert("CMYK"), quality=90)
    data = bytearray(save(small, quality=90, subsampling=1))   # 4:2:2 with the luma factors swapped: 4:4:0
    at = data.index(b"\xff\xc0")
    assert data[at + 11] == 0x21
    data[at + 11] = 0x12
    out["refuse_440"] = bytes(data)
    return out


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, data in sorted(files().items()):
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        total += len(data)
    print(len(files()), "files,", total, "bytes")
