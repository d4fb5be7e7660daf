"""CPU: the contrast-enhancement rule of include/codetr_enhance.h -- the binder and the header's constants, what
enhance_settings completes and refuses, the host checks stand-alone under the sanitizers, the redistribution's closed form
against the literal loop, and the restatement tests/enhance_ref.py within the header's derived bound of float64."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import enhance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binder_constants_and_names():
    from codetr import _cabi, _enhance, hip_ops
    from codetr.inferencer import enhance_call_settings

    assert _enhance.ABI_VERSION == 1 and _enhance.load().codetr_enhance_abi_version() == 1 and _cabi.CALLS["enhance"] >= 0
    assert (_enhance.ROW_INTS, _enhance.MAX_GRID, _enhance.MAX_TILE, _enhance.SLICE_PIXELS, _enhance.MAX_SLICES) == (9, 32, 1 << 22, 8192, 32)
    assert hip_ops.ENHANCE_MAX_GRID == 32 and hip_ops.ENHANCE_DEFAULTS == dict(grid=(8, 8), clip_limit=2.0)
    assert hip_ops.enhance_frames.__module__ == hip_ops.enhance_settings.__module__ == "codetr.enhance_ops"
    # 1080p at 8 x 8: tiles of 135 x 240 in 4 slices, 1 KB each; the geometry is the library's own
    assert _enhance.workspace_bytes([(1080, 1920, 0, 5760, 0, 5760, 8, 8, 253)] * 2) == 2 * 64 * 4 * 1024
    with pytest.raises(RuntimeError):
        _enhance.workspace_bytes([(1080, 1920, 0, 5760, 0, 5760, 33, 8, 1)])
    assert enhance_call_settings(None, 3) is None and len(enhance_call_settings({}, 3)) == 3
    with pytest.raises(ValueError, match="2 values for 3"):
        enhance_call_settings([{}, {}], 3)


@pytest.mark.parametrize("given, size, want", [
    ({}, None, dict(grid=(8, 8), clip_limit=2.0)),
    (dict(grid=[1, 32], clip_limit=None), (7, 64), dict(grid=(1, 32), clip_limit=None, clip_count=14)),
    (dict(clip_limit=2), (1080, 1920), dict(grid=(8, 8), clip_limit=2.0, clip_count=253)),      # (512 * 32400) >> 16
    (dict(clip_limit=1 / 256, grid=(np.int64(2), 2)), (9, 9), dict(grid=(2, 2), clip_limit=1 / 256, clip_count=1)),
    (dict(clip_limit=256.0, grid=(1, 1)), (2048, 2048), dict(grid=(1, 1), clip_limit=256.0, clip_count=1 << 22)),
])
def test_settings_accepted(given, size, want):
    from codetr import hip_ops

    s = hip_ops.enhance_settings(given, *(size or ()))
    assert s == want and hip_ops.enhance_settings(s, *(size or ())) == s
    if size:
        assert s["clip_count"] == R.clip_count(s["clip_limit"], -(-size[0] // s["grid"][0]) * -(-size[1] // s["grid"][1]))


@pytest.mark.parametrize("bad, size, match", [
    (None, None, "a dict"), (dict(tiles=8), None, "unknown key"), (dict(grid=8), None, "grid"), (dict(grid=(0, 8)), None, "grid"),
    (dict(grid=(8, 33)), None, "grid"), (dict(grid=(8.0, 8)), None, "grid"), (dict(grid=(8, 8, 8)), None, "grid"),
    (dict(clip_limit=0.003), None, "clip_limit"), (dict(clip_limit=256.5), None, "clip_limit"), (dict(clip_limit="2"), None, "clip_limit"),
    (dict(clip_limit=float("nan")), None, "clip_limit"), (dict(clip_limit=True), None, "clip_limit"),
    (dict(grid=(8, 8)), (7, 64), "more tiles"), (dict(grid=(1, 1)), (2048, 2049), "at most"),
])
def test_settings_refused(bad, size, match):
    from codetr import hip_ops

    with pytest.raises(ValueError, match=match):
        hip_ops.enhance_settings(bad, *(size or ()))


def test_host_checks_memory_check(tmp_path):
    """csrc/enhance_args.h on the host under -fsanitize=address,undefined (a stand-alone program, nothing preloaded)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "enhance_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "enhance_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)   # no sanitizer runtimes here: the answers still hold
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == "checks ok clean".split(), r.stdout + r.stderr[-2000:]


@pytest.mark.parametrize("C", [1, 7, 300])
def test_redistribution_closed_form_equals_the_loop(C):
    """every residual r in 0..255 (and several batches E >> 8): OpenCV's loop, written out, against step 5"""
    rng = np.random.default_rng(C)
    seen = set()
    for E in list(range(256)) + [256, 511, 1000, 70001]:
        h = np.minimum(rng.integers(0, C + 1, 256), C)
        h[rng.integers(0, 256)] = C + E                      # the excess is exactly E
        want, r = np.minimum(h, C) + E // 256, E % 256
        if r:
            i, step = 0, max(256 // r, 1)
            while i < 256 and r > 0:
                want[i] += 1
                i, r = i + step, r - 1
        got = R.redistribute(h, C)
        assert np.array_equal(got, want) and got.sum() == h.sum(), E
        seen.add(E % 256)
    assert seen == set(range(256))


@pytest.mark.parametrize("size, grid, clip_limit", [((37, 150), (4, 8), 2.0), ((64, 48), (8, 8), None), ((9, 9), (9, 9), 1 / 256),
                                                    ((50, 31), (1, 1), 40.0), ((23, 57), (3, 32), 0.5)])
def test_restatement_within_the_derived_bound_of_float64(size, grid, clip_limit):
    """the header derives |out - out_real| <= CODETR_ENHANCE_BOUND_HALVES / 2 = 1; images with a narrow tonal range, where the
    tables are steep, and random ones"""
    from codetr import _enhance

    rng = np.random.default_rng(size[0])
    narrow = np.clip(rng.normal(90, 6, size + (3,)), 0, 255).astype(np.uint8)
    for image in (narrow, rng.integers(0, 256, size + (3,), dtype=np.uint8)):
        got, real = R.enhance(image, grid, clip_limit), R.enhance(image, grid, clip_limit, real=True)
        err = np.abs(got.astype(np.float64) - real).max()
        print(size, grid, clip_limit, "max |out - real| =", err)
        assert got.dtype == np.uint8 and got.shape == image.shape and err <= _enhance.BOUND_HALVES / 2 + 1e-9
    assert (got != image).any()
