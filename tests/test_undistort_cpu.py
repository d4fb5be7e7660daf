"""CPU: the lens rule of include/codetr_undistort.h -- the binder and the header's constants, what undistort_settings
completes and refuses, the host checks stand-alone under the sanitizers, the header's ATAN and its two derived bounds
against float64, the identity, and distort_points against the restatement tests/undistort_ref.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import undistort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERAS = {   # mild calibrations of a 97 x 131 frame, new_camera_matrix a little off the camera's
    "brown": dict(model="brown", camera_matrix=(88.0, 91.0, 64.3, 47.9), dist_coeffs=(-0.21, 0.07, 0.004, -0.003, -0.01, 0.02, -0.03, 0.01)),
    "fisheye": dict(model="fisheye", camera_matrix=(61.0, 60.0, 66.1, 49.2), dist_coeffs=(-0.03, 0.011, -0.004, 0.0009)),
}


def test_binder_constants_and_settings():
    from codetr import _cabi, _undistort, hip_ops

    assert _undistort.ABI_VERSION == 1 and _undistort.load().codetr_undistort_abi_version() == 1 and "undistort" in _cabi.CALLS
    assert (_undistort.ROW_INTS, _undistort.PARAM_FLOATS, _undistort.MAX_FOCAL, _undistort.MAX_CENTRE) == (9, 16, 16384, 32768)
    assert hip_ops.UNDISTORT_MODELS == {"brown": 0, "fisheye": 1} and hip_ops.undistort_frames.__module__ == "codetr.undistort_ops"
    assert hip_ops.UNDISTORT_DEFAULTS == dict(model="brown", camera_matrix=None, dist_coeffs=(), new_camera_matrix=None,
                                              size=None, fill=(0, 0, 0))
    s = hip_ops.undistort_settings(dict(camera_matrix=[[800.1, 0, 320], [0, 801, 240], [0, 0, 1]], dist_coeffs=np.array([[0.1, 0, 0, 0, 0.3]])), 480, 640)
    assert s["camera_matrix"] == s["new_camera_matrix"] == (800.1, 801.0, 320.0, 240.0) and s["size"] == (480, 640) and s["code"] == 0
    assert s["params"] == (float(np.float32(800.1)), 801.0, 320.0, 240.0) * 2 + (float(np.float32(0.1)), 0.0, 0.0, 0.0, float(np.float32(0.3)), 0.0, 0.0, 0.0)
    assert hip_ops.undistort_settings(s) == s and hip_ops.undistort_settings(dict(camera_matrix=(1, 1, 0, 0)))["size"] is None
    cam = (100.0, 100.0, 5.0, 5.0)
    for bad, match in [(None, "a dict"), ({}, "camera_matrix is required"), (dict(camera_matrix=[[1, 0.1, 0], [0, 1, 0], [0, 0, 1]]), "skew"),
                       (dict(camera_matrix=(0.0, 1, 0, 0)), "camera_matrix"), (dict(camera_matrix=(1, 16385, 0, 0)), "camera_matrix"),
                       (dict(camera_matrix=(1, 1, float("nan"), 0)), "camera_matrix"), (dict(camera_matrix=(1, 1, 0, 32769)), "camera_matrix"),
                       (dict(camera_matrix=cam, new_camera_matrix=(1, -1, 0, 0)), "new_camera_matrix"), (dict(camera_matrix=cam, model="pinhole"), "model"),
                       (dict(camera_matrix=cam, dist_coeffs=(0.1,) * 6), "0 or 4 or 5 or 8"), (dict(camera_matrix=cam, dist_coeffs=(0.1,) * 5, model="fisheye"), "0 or 4"),
                       (dict(camera_matrix=cam, dist_coeffs=(0.1, float("inf"), 0, 0)), "dist_coeffs"), (dict(camera_matrix=cam, size=(0, 5)), "size"),
                       (dict(camera_matrix=cam, size=(5, 32768)), "size"), (dict(camera_matrix=cam, fill=(0, 0, 256)), "fill"),
                       (dict(camera_matrix=cam, border="reflect"), "unknown key")]:
        with pytest.raises(ValueError, match=match):
            hip_ops.undistort_settings(bad)


def test_host_checks_memory_check(tmp_path):
    """csrc/undistort_args.h on the host under -fsanitize=address,undefined (a stand-alone program, nothing preloaded)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "undistort_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "undistort_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)   # no sanitizer runtimes here: the answers still hold
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == "checks ok clean".split(), r.stdout + r.stderr[-2000:]


def test_atan_within_the_header_s_distance_of_float64():
    """a dense grid of [0, 1e8] and every fp32 within 4096 ulps of the reduction point 1; the header's criterion at the
    largest admitted focal length"""
    from codetr import _undistort

    near = (np.float32(1).view(np.int32) + np.arange(-4096, 4097, dtype=np.int32)).view(np.float32)
    r = np.concatenate([np.linspace(0, 1, 2000001), np.linspace(1, 40, 2000001), np.logspace(0, 8, 200001)]).astype(np.float32)
    err = max(np.abs(R.atan(g).astype(np.float64) - np.arctan(g.astype(np.float64))).max() for g in (near, r))
    print("max |ATAN - atan| =", err, "header: 1.91e-7, DELTA", R.DELTA)
    assert err <= 1.91e-7 < R.DELTA and _undistort.MAX_FOCAL * R.DELTA <= (1 / 32) / 4 / 2
    assert R.atan(np.float32([0, 1]))[0] == 0 and abs(float(R.atan(np.float32([1]))[0]) - math.pi / 4) <= R.DELTA


@pytest.mark.parametrize("model", ["brown", "fisheye"])
def test_derived_bounds_and_distort_points_against_float64(model):
    """random calibrations inside the admitted ranges: bound 1 at every valid pixel, against distort_points too; bound 2 on
    a random image, against the real bilinear interpolation at the real position"""
    from codetr import hip_ops

    rng = np.random.default_rng(7 + len(model))
    H, W, Ho, Wo = 97, 131, 75, 120
    for trial in range(12):
        f = float(rng.uniform(40, 400) if trial else 16384.0)          # (the first: the largest focal length)
        coeffs = rng.uniform(-1, 1, 8 if model == "brown" else 4) * ([0.3, 0.1, 0.01, 0.01, 0.05, 0.3, 0.1, 0.05] if model == "brown" else [0.1, 0.03, 0.01, 0.003])
        s = hip_ops.undistort_settings(dict(model=model, camera_matrix=(f, f * rng.uniform(0.8, 1.0), W * rng.uniform(0.3, 0.7), H * rng.uniform(0.3, 0.7)),
                                            new_camera_matrix=(min(16384.0, f * rng.uniform(0.4, 1.5)), f * rng.uniform(0.4, 1.0), Wo / 2 + rng.uniform(-9, 9), Ho / 2),
                                            dist_coeffs=coeffs, size=(Ho, Wo), fill=(9, 200, 77)))
        X, Y, valid = R.positions(s["params"], model, Ho, Wo)
        v, u = np.mgrid[0:Ho, 0:Wo]
        us, vs, Ex, Ey = R.real_and_bound(s["params"], model, u, v)
        dx, dy = np.abs(X / 32 - us)[valid], np.abs(Y / 32 - vs)[valid]
        print(model, trial, "max |X/32 - us| - 1/64 =", (dx.max() - 1 / 64), "E up to", Ex[valid].max())
        assert valid.any() and (dx <= 1 / 64 + Ex[valid]).all() and (dy <= 1 / 64 + Ey[valid]).all()
        pts = hip_ops.distort_points(np.stack([u.ravel(), v.ravel()], 1), s).reshape(Ho, Wo, 2)
        assert np.abs(pts[..., 0] - us).max() <= 1e-9 * (1 + np.abs(us).max()) and np.abs(pts[..., 1] - vs).max() <= 1e-9 * (1 + np.abs(vs).max())
        # bound 2: the stored image continued by `fill`, one pixel of it on every side of all the taps
        image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ok = valid & (us > -1) & (us < W) & (vs > -1) & (vs < H)
        big = np.empty((H + 4, W + 4, 3), np.float64)
        big[...] = s["fill"]
        big[2:-2, 2:-2] = image
        D = max(np.abs(np.diff(big, axis=0)).max(), np.abs(np.diff(big, axis=1)).max())
        x0, y0 = np.floor(us[ok]).astype(int), np.floor(vs[ok]).astype(int)
        a, b = (us[ok] - x0)[:, None], (vs[ok] - y0)[:, None]
        real = ((1 - a) * (1 - b) * big[y0 + 2, x0 + 2] + a * (1 - b) * big[y0 + 2, x0 + 3] + (1 - a) * b * big[y0 + 3, x0 + 2] + a * b * big[y0 + 3, x0 + 3])
        err = np.abs(R.remap(image, s)[ok].astype(np.float64) - real).max(axis=1)
        assert (err <= 0.5 + D * (1 / 32 + Ex[ok] + Ey[ok])).all()


def test_identity_calibration_returns_the_input():
    """zero coefficients, the camera's own matrix and size: X = 32 u at the ends of the admitted ranges"""
    from codetr import hip_ops

    image = np.random.default_rng(1).integers(0, 256, (61, 83, 3), dtype=np.uint8)
    for cam in [(700.3, 655.1, 41.7, 30.2), (16384.0, 0.013, -32768.0, 32768.0), (3.3, 16384.0, 32768.0, -32768.0)]:
        s = hip_ops.undistort_settings(dict(camera_matrix=cam), 61, 83)
        assert np.array_equal(R.remap(image, s), image), cam
        X, Y, valid = R.positions(s["params"], "brown", 2, 32767)     # the widest frame there can be
        assert valid.all() and np.array_equal(X[1], 32 * np.arange(32767)) and np.array_equal(Y[:, 5], [0, 32])
