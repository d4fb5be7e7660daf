"""CPU: the raw Bayer rule of include/codetr_raw.h -- the restatement tests/raw_ref.py against the same computation in
float64 within the header's derived bound, the identity of the default settings, what the settings and the frame parser
refuse, the host side (fold, multipliers, the entry point's checks) stand-alone under the sanitizers, and Malvar against bilinear
on a smooth image."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import raw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# include/codetr_raw.h, "How far the rule is ...": 0.5 + 255 (15 + E) / 65535 with E = 3.0 (malvar), 1.5 (bilinear)
BOUND = {"malvar": 0.5 + 255 * (15 + 3.0) / 65535, "bilinear": 0.5 + 255 * (15 + 1.5) / 65535}


@pytest.mark.parametrize("bits", [8, 12, 16])
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
@pytest.mark.parametrize("method", ["malvar", "bilinear"])
def test_restatement_within_the_derived_bound_of_float64(method, pattern, bits):
    rng = np.random.default_rng(bits + R.PATTERNS[pattern])
    s = rng.integers(0, 2 ** bits, (37, 41))
    s[:8] = rng.integers(0, 2, (8, 41)) * (2 ** bits - 1)   # rows of extremes: the filters' clamps at work
    levels = dict(black_level=2 ** bits // 16, white_level=2 ** bits - 2 ** bits // 8, white_balance=(1.9, 1.0, 1.4))
    for kw in (dict(bits=bits, method=method), dict(bits=bits, method=method, **levels)):
        err = np.abs(R.demosaic(s, pattern, **kw).astype(np.float64) - R.demosaic(s, pattern, real=True, **kw)).max()
        print(method, pattern, bits, "max |rule - real| =", err, "bound", BOUND[method])
        assert err <= BOUND[method]


def test_default_settings_keep_a_site_s_own_colour():
    from codetr import hip_ops

    assert np.array_equal(hip_ops.raw_settings()["lut"], R.LINEAR)
    s = np.arange(256).reshape(16, 16)
    assert np.array_equal(R.demosaic(s, "bayer_rggb")[::2, ::2, 0], s[::2, ::2])      # red sites: the input byte
    for bits, slack in [(8, 0), (10, 0), (12, 0), (14, 1), (16, 1)]:   # a flat frame is its own colour at every site
        v = np.arange(2 ** bits)
        out = R.demosaic(np.repeat(v[:, None], 2, 1), "bayer_grbg", bits=bits)[:, 0, 1]
        assert np.abs(out - np.floor(v * 255 / (2 ** bits - 1) + 0.5)).max() <= slack, bits


def test_settings_and_parser_refusals():
    from codetr import _raw, hip_ops
    from codetr.inferencer import frame_settings, parse_frame

    assert _raw.ABI_VERSION == 1 and _raw.load().codetr_raw_abi_version() == 1 and hip_ops.RAW_FORMATS == R.PATTERNS
    assert "bayer_rggb" not in hip_ops.FRAME_FORMATS and set(hip_ops.RAW_METHODS) == {"malvar", "bilinear"}
    s = hip_ops.raw_settings(dict(bits=12, black_level=64, white_balance=(2.0, 1.0, 1.5), tone="srgb"))
    assert s["operands"] == (0, 64, 4095) + tuple(R.multipliers(64, 4095, (2.0, 1.0, 1.5))) and s["lut"][[0, 4095]].tolist() == [0, 255]
    assert frame_settings("bayer_bggr")["raw"]["operands"] == (0, 0, 255) + (257 * 65536,) * 3 and "raw" not in frame_settings("gray")
    for bad, match in [(dict(black_level=255), "white_level"), (dict(bits=10, white_level=1024), "white_level"),
                       (dict(white_level=1, white_balance=(1.0, 65537.0, 1.0)), r"2\*\*32"), (dict(method="vng"), "method"),
                       (dict(tone=np.zeros(256, np.uint8)), "tone"), (dict(gamma=2.2), "unknown key")]:
        with pytest.raises(ValueError, match=match):
            hip_ops.raw_settings(bad)
    with pytest.raises(ValueError, match="raw="):
        frame_settings("nv12", raw=dict(bits=8))
    assert parse_frame(np.zeros((5, 7), np.uint16), "bayer_rggb", 12).planes[0].shape == (5, 14)
    for item, bits in [(np.zeros((5, 7), np.uint16), 8), (np.zeros((5, 7, 1), np.uint8), 8), (np.zeros((5, 7), np.uint8), 12)]:
        with pytest.raises(ValueError, match="bayer_rggb"):   # (the last: 7 bytes a row are no 16-bit samples)
            parse_frame(item, "bayer_rggb", bits)


def test_host_side_memory_check(tmp_path):
    """csrc/raw_args.h on the host under -fsanitize=address,undefined (a stand-alone program, nothing preloaded)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "raw_args_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "raw_args_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)   # no sanitizer runtimes here: the answers still hold
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == "fold ok multipliers ok checks ok clean".split(), r.stdout + r.stderr[-2000:]


@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_malvar_beats_bilinear_on_a_smooth_image(pattern):
    yy, xx = np.mgrid[0:96, 0:128]
    y, x = yy / 16.0, xx / 16.0
    luma = 0.5 + 0.2 * np.sin(1.3 * x + 0.4 * y) + 0.15 * np.sin(0.7 * y - 0.9 * x + 1.0) + 0.1 * np.sin(2.1 * y)
    rgb = np.round(255 * np.clip(np.stack([luma * 0.9, luma, luma * 0.8 + 0.05 * np.sin(0.5 * x)], -1), 0, 1)).astype(np.int64)
    ry, rx = divmod(R.PATTERNS[pattern], 2)
    channel = np.where((yy % 2 == ry) & (xx % 2 == rx), 0, np.where((yy % 2 != ry) & (xx % 2 != rx), 2, 1))
    mosaic = np.take_along_axis(rgb, channel[..., None], 2)[..., 0]
    psnr = {m: 10 * np.log10(255.0 ** 2 / np.mean((R.demosaic(mosaic, pattern, method=m).astype(np.float64) - rgb) ** 2))
            for m in ("malvar", "bilinear")}
    print(pattern, psnr)
    assert psnr["malvar"] > psnr["bilinear"]
