"""The case list of the JPEG decoder tests: the committed files of tests/golden/jpeg_dec (written by
tools/gen_jpeg_dec_fixtures.py with Pillow), the five corrupt scans, and what the restatement (jpeg_dec_ref.py) makes of
them -- decoded once per process and shared."""
import functools
import os

import numpy as np

import jpeg_dec_ref as D

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_dec")
NAMES = sorted(f[:-4] for f in os.listdir(DIR) if f.endswith(".jpg"))
REFUSED = {"refuse_progressive": "progressive", "refuse_cmyk": "components", "refuse_440": "sampling"}
SUPPORTED = [n for n in NAMES if n not in REFUSED]
GROUPS = ("444", "422", "420", "grey")
NOISE, GRADIENT = "420_320x240_noise_q90", "420_320x240_gradient_q90_rr1"


def group(sub):
    return [n for n in SUPPORTED if n.startswith(sub + "_")]


@functools.lru_cache(maxsize=None)
def data(name):
    with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(rgb, status, stats) of the restatement; the arrays are shared: do not write to them"""
    stats = {}
    rgb, status = D.decode(data(name) if name in NAMES else corrupt()[name], stats)
    rgb.setflags(write=False)
    return rgb, status, stats


def _patched(name, edit):
    """the file with its scan bytes edited: edit(bytearray of the scan) -> new scan"""
    raw = data(name)
    info = D.parse(raw)
    a, n = info["scan_offset"], info["scan_bytes"]
    return raw[:a] + bytes(edit(bytearray(raw[a:a + n]))) + raw[a + n:]


@functools.lru_cache(maxsize=None)
def corrupt():
    """five corrupt scans, each a fixed edit of a committed file: bit flips, a cut scan, a wrong RST number, a marker
    where none belongs.  They show the status path; every one decodes to a status in the restatement and in the host
    memory check (test_jpeg_dec_cpu.py runs it over these bytes)."""
    def flip(at_bits):
        def edit(s):
            for byte, bit in at_bits:
                s[byte % len(s)] ^= 1 << bit
            return s
        return edit

    def renumber(s):
        at = s.index(b"\xff\xd0")
        s[at + 1] = 0xD3
        return s

    def stray(s):
        s[len(s) // 2:len(s) // 2 + 2] = b"\xff\xd5"
        return s

    return {
        "corrupt_flip_420": _patched("420_33x31_q90", flip([(200, 3)])),
        "corrupt_flips_444": _patched("444_37x53_q100", flip([(100, 7), (3000, 0), (3001, 5), (7000, 2)])),
        "corrupt_cut_422": _patched("422_37x53_q90", lambda s: s[:len(s) // 2]),
        "corrupt_rst_number_444": _patched("444_17x9_q30_rr1", renumber),
        "corrupt_stray_rst_420": _patched("420_5x40_q90", stray),
    }


def encoder_image():
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[:160, :40]
    im = np.clip(np.stack([xx * 6 + yy, yy + 40, 250 - xx * 5], -1) % 256 + rng.integers(-9, 10, (160, 40, 3)), 0, 255)
    return im.astype(np.uint8)


def encoder_file():
    """the project's own encoder (jpeg_ref.encode): one restart interval per MCU row, 10 rows, so the RST numbering wraps"""
    import jpeg_ref

    return jpeg_ref.encode(encoder_image(), 90, "420")
