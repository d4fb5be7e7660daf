#!/usr/bin/env python3
"""Write tests/golden/orient/*.jpg: thirteen baseline JPEGs of 17 x 9 pixels (Pillow's encoder, 4:2:0 and 4:4:4 in turn, every
one inside the GPU decoder's supported set) with a hand-built Exif APP1 segment behind SOI -- the cases of
tests/test_orient_cpu.py and tests/test_orient_gpu.py.  The name says what the reader must return: `o<k>_...` is k, any
other name 1.
    o1..o8_be   tag 0x0112, SHORT, count 1, big-endian TIFF ("MM"), behind an ImageWidth entry
    o6_le, o8_le  the same in little-endian ("II")
    none        no Exif segment
    long6_le    the tag typed LONG (little-endian, so that a reader that ignores the type would see 6)
    badifd6_be  an IFD0 offset that points outside the segment
    python tools/gen_orient_fixtures.py"""
import io
import os
import struct

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "orient")
H, W = 9, 17


def picture():
    """a smooth picture whose four corners differ, so that every orientation gives another image"""
    y, x = np.mgrid[0:H, 0:W]
    rgb = np.stack([40 + 12 * x, 30 + 24 * y, 250 - 9 * x - 8 * y], axis=-1)
    rgb[1:4, 2:6] = (250, 20, 20)
    return rgb.astype(np.uint8)


def exif(value, little=False, kind=3, ifd=8):
    e = "<" if little else ">"
    entry = struct.pack(e + "HHI", 0x0112, kind, 1) + (struct.pack(e + "HH", value, 0) if kind == 3 else struct.pack(e + "I", value))
    tiff = (b"II*\0" if little else b"MM\0*") + struct.pack(e + "I", ifd) + struct.pack(e + "H", 2) + \
        struct.pack(e + "HHIHH", 0x0100, 3, 1, W, 0) + entry + struct.pack(e + "I", 0)
    payload = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def main():
    os.makedirs(OUT, exist_ok=True)
    cases = [(f"o{k}_be", exif(k)) for k in range(1, 9)]
    cases += [("o6_le", exif(6, little=True)), ("o8_le", exif(8, little=True)), ("none", b""),
              ("long6_le", exif(6, little=True, kind=4)), ("badifd6_be", exif(6, ifd=4000))]
    for i, (name, segment) in enumerate(cases):
        sub = ("420", "444")[i % 2]
        buf = io.BytesIO()
        Image.fromarray(picture()).save(buf, "JPEG", quality=90, subsampling=dict([("420", 2), ("444", 0)])[sub])
        data = buf.getvalue()
        assert data[:2] == b"\xff\xd8"
        with open(os.path.join(OUT, f"{name}_{sub}.jpg"), "wb") as f:
            f.write(data[:2] + segment + data[2:])
    print(OUT, len(cases))


if __name__ == "__main__":
    main()
