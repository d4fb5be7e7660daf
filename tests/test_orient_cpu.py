"""CPU: the orientation rule of include/codetr_orient.h -- the EXIF reader on the files of tests/golden/orient
(tools/gen_orient_fixtures.py) and, stand-alone under the sanitizers, on every prefix of them; the entry point's refusals,
which come before any HIP call; the settings and the box helper.  TABLE is the reference, of test_orient_gpu.py too."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "orient")
NAMES = sorted(f[:-4] for f in os.listdir(DIR) if f.endswith(".jpg"))
TABLE = {   # out[y'][x'] = in[y][x]: the header's eight rows, on [H, W, 3] arrays
    1: lambda a: a,                                  # (y, x)
    2: lambda a: a[:, ::-1],                         # (y, W-1-x)
    3: lambda a: a[::-1, ::-1],                      # (H-1-y, W-1-x)
    4: lambda a: a[::-1],                            # (H-1-y, x)
    5: lambda a: a.transpose(1, 0, 2),               # (x, y)
    6: lambda a: a[::-1].transpose(1, 0, 2),         # (x, H-1-y)
    7: lambda a: a[::-1, ::-1].transpose(1, 0, 2),   # (W-1-x, H-1-y)
    8: lambda a: a[:, ::-1].transpose(1, 0, 2),      # (W-1-x, y)
}


def data(name):
    return open(os.path.join(DIR, name + ".jpg"), "rb").read()


def expected(name):   # the generator's names say what the reader must return
    return int(name[1]) if name[0] == "o" else 1


def test_reader_on_the_committed_files_and_pillow():
    """the reader's value per file; where Pillow imports, table and reader against ImageOps.exif_transpose -- but for
    `long6`, the tag typed LONG: Pillow takes a value of any integer type, the header's rule SHORT only"""
    from codetr import _cabi, _orient, hip_ops

    assert _orient.ABI_VERSION == 1 and _orient.load().codetr_orient_abi_version() == 1 and "orient" in _cabi.CALLS
    assert len(NAMES) == 13 and {expected(n) for n in NAMES} == set(range(1, 9))
    for name in NAMES:
        assert hip_ops.jpeg_orientation(data(name)) == expected(name), name
        assert hip_ops.jpeg_info(data(name))["supported"], name            # the GPU decoder takes every one of them
    assert _orient.load().codetr_orient_exif(None, 5) == -1 and _orient.load().codetr_orient_exif(ctypes.c_void_p(16), 0) == -1
    assert hip_ops.oriented_size(3, 9, 17) == (9, 17) and hip_ops.oriented_size(6, 9, 17) == (17, 9)
    Image, ImageOps = pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageOps")
    for name in (n for n in NAMES if not n.startswith("long")):
        stored = Image.open(io.BytesIO(data(name)))
        upright = np.asarray(ImageOps.exif_transpose(stored).convert("RGB"))
        assert np.array_equal(upright, TABLE[expected(name)](np.asarray(stored.convert("RGB")))), name


def test_reader_host_memory_check(tmp_path):
    """the reader on the host under -fsanitize=address,undefined (a stand-alone program, nothing preloaded): every file and
    every prefix of every file, each in a heap block of exactly its length"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, files = str(tmp_path / "orient_exif_host_check"), [os.path.join(DIR, n + ".jpg") for n in NAMES]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "orient_exif_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if (subprocess.run(cmd + san, capture_output=True).returncode != 0
            or subprocess.run([exe, files[0]], capture_output=True).returncode != 0):
        subprocess.run(cmd, check=True, capture_output=True)   # no sanitizer runtimes here: the answers still hold
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("clean"), r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.split()[:-1] == [v for n in NAMES for v in (n + ".jpg", str(expected(n)))]


def test_entry_point_refuses_before_any_hip_call():
    from codetr import _cabi, _orient

    lib, src, dst = _orient.load(), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    big, good = _cabi.FRAME_MAX_SIDE + 1, (6, 4, 5, 0, 15, 0)

    def call(rows, src=src, dst=dst, N=None):
        flat = (ctypes.c_int64 * (6 * len(rows)))(*[v for r in rows for v in r])
        return lib.codetr_orient_rgb_u8(None, src, 4096, len(rows) if N is None else N, flat, dst, 4096)

    for rows, kw, code in [
            ([(0,) + good[1:]], {}, -1), ([(9,) + good[1:]], {}, -1),                  # o outside 1..8
            ([good, (3, 4, 5, 100, 15, 59)], {}, -1),                                  # the outputs share byte 59
            ([(6, 4, 5, 0, 14, 0)], {}, -1),                                           # a pitch below 3 W
            ([(6, 4, 5, 4096 - 59, 15, 0)], {}, -1), ([(6, 4, 5, 0, 15, 4096 - 59)], {}, -1),   # one byte outside
            ([(6, 0, 5, 0, 15, 0)], {}, -1), ([good], dict(N=0), -1), ([good], dict(src=None), -1), ([good], dict(dst=None), -1),
            ([good], dict(dst=ctypes.c_void_p((1 << 20) + 4095)), -1),                 # src and dst share a byte
            ([(6, big, 1, 0, 3, 0)], {}, -3), ([(1, 1, big, 0, 3 * big, 0)], {}, -3),  # a side above the limit
            ([good] * 33, {}, -3)]:
        assert call(rows, **kw) == code, (rows, kw)


def test_orientation_settings():
    from codetr.inferencer import orientation_settings

    assert orientation_settings(None, 3) is None and orientation_settings(6, 3) == [6, 6, 6]
    assert orientation_settings([1, np.int64(8), 3], 3) == [1, 8, 3] and orientation_settings("exif", 2, "jpeg") == "exif"
    for bad, fmt, match in [(0, "rgb", "1..8"), (9, "rgb", "1..8"), (True, "rgb", "1..8"), (6.0, "rgb", "1..8"),
                            ("auto", "jpeg", "1..8"), ([6, 6], "rgb", "2 values for 3"), ([6, "exif", 1], "jpeg", "1..8"),
                            ("exif", "rgb", "input_format"), ("exif", "nv12", "input_format")]:
        with pytest.raises(ValueError, match=match):
            orientation_settings(bad, 3, fmt)


@pytest.mark.parametrize("o", range(1, 9))
def test_unorient_boxes_round_trips_against_the_table(o):
    """a box of whole pixels, marked in the stored image and found again in the upright one, maps back to itself"""
    from codetr import hip_ops

    stored = np.zeros((9, 17, 3), np.uint8)
    stored[1:5, 2:7] = 1
    ys, xs = np.nonzero(TABLE[o](stored)[..., 0])
    upright = [[xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]]
    assert hip_ops.unorient_boxes(upright, o, 9, 17).tolist() == [[2.0, 1.0, 7.0, 5.0]]
