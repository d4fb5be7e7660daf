"""GPU: codetr_undistort_rgb_u8 (csrc/undistort.hip), hip_ops.undistort_frames and `Inferencer(...)(..., undistort=...)` byte
for byte against the restatement tests/undistort_ref.py (the rule is exact: no tolerance)."""
import numpy as np
import pytest
import torch

import frames_ref as FR
import undistort_ref as R
from test_inferencer_batch_gpu import DEV
from test_jpeg_gpu import PATHS, _inferencer, _items
from test_orient_cpu import TABLE

pytestmark = pytest.mark.gpu
GUARD = 48
TW, TH, BUDGET = 64, 16, 4864   # the kernel's output tile and its LDS window, in dwords
# a pixel, a row, a column, one below / at / above the tile on each axis, ragged tiles on both axes
SIZES = [(1, 1), (1, TW + 3), (TH + 3, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (37, 150)]
CALL = dict(batch_size=3, pred_score_thr=0.4, device=DEV, dtype=torch.float16, return_vis=True)
COEFFS = {"brown": dict(mild=(-0.12, 0.03, 0.002, -0.001, 0.004), strong=(-0.9, 0.6, 0.05, -0.04, 0.2, 0.3, -0.2, 0.1)),
          "fisheye": dict(mild=(-0.02, 0.004, -0.001, 0.0002), strong=(0.9, -0.2, 0.5, 0.1))}


def _camera(model, kind, H, W, Ho, Wo):
    """a calibration of a stored H x W frame for an Ho x Wo rectified image: `mild`; `strong`, which sends part of the image
    to a non-black fill; `zoom`, fx' a third of fx, so that a whole output tile needs 3 x 3 times its own area of source"""
    from codetr import hip_ops

    f = 0.8 * max(H, W, 8)
    cam = (f, 0.97 * f, 0.52 * W, 0.47 * H)
    new = {"mild": (0.9 * f * Wo / W, 0.9 * f * Ho / H, 0.5 * Wo, 0.5 * Ho), "strong": (0.3 * f, 0.3 * f, 0.4 * Wo, 0.6 * Ho),
           "zoom": (f / 3, 0.97 * f / 3, 0.52 * W / 3, 0.47 * H / 3)}[kind]
    return hip_ops.undistort_settings(dict(model=model, camera_matrix=cam, new_camera_matrix=new, size=(Ho, Wo),
                                           dist_coeffs=COEFFS[model]["mild" if kind == "zoom" else kind],
                                           fill=(200, 30, 90) if kind == "strong" else (0, 0, 0)))


def _launch(frames, seed=3):
    """frames [(image, settings)] at odd offsets with pitches 3 W + {0, 1, 5} and random bytes between, one call of the entry
    point into slots at both residues (a multiple of 4, and not) with 0xA5 guard bytes around them -> the rectified images"""
    from codetr import _undistort

    rows, at, dst = [], 1, GUARD
    for k, (im, s) in enumerate(frames):
        (H, W), (Ho, Wo), (r, g, b) = im.shape[:2], s["size"], s["fill"]
        dst += (k % 2 - dst) % 4            # even frames at a multiple of 4, odd ones one byte behind it
        rows.append((s["code"], H, W, at, 3 * W + (0, 1, 5)[k % 3], Ho, Wo, dst, r << 16 | g << 8 | b))
        at += H * rows[-1][4] + 2
        at += 1 - at % 2                    # (every offset odd)
        dst += Ho * Wo * 3 + GUARD
    src = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)
    for (_, H, W, off, pitch, *_), (im, _) in zip(rows, frames):
        for y in range(H):
            src[off + y * pitch:off + y * pitch + 3 * W] = im[y].reshape(-1)
    dev = torch.from_numpy(src).to(DEV)
    out = torch.full((dst,), 0xA5, dtype=torch.uint8, device=DEV)
    _undistort.remap(dev, rows, [s["params"] for _, s in frames], out)
    host, images = out.cpu().numpy(), []
    assert np.array_equal(dev.cpu().numpy(), src)          # the stored frames are only read
    for _, _, _, _, _, Ho, Wo, d, _ in rows:
        images.append(host[d:d + Ho * Wo * 3].reshape(Ho, Wo, 3).copy())
        host[d:d + Ho * Wo * 3] = 0xA5
    assert (host == 0xA5).all(), "guard bytes around an image were written"
    return images


def _over_budget(im, s):
    """per output tile that samples the frame at all: whether its source window exceeds the LDS budget (the direct path)"""
    (H, W), (Ho, Wo) = im.shape[:2], s["size"]
    X, Y, valid = R.positions(s["params"], s["model"], Ho, Wo)
    xi, yi = X >> 5, Y >> 5
    live, over = valid & (xi >= -1) & (xi < W) & (yi >= -1) & (yi < H), []
    for ty in range(0, Ho, TH):
        for tx in range(0, Wo, TW):
            m = live[ty:ty + TH, tx:tx + TW]
            if m.any():
                x, y = xi[ty:ty + TH, tx:tx + TW][m], yi[ty:ty + TH, tx:tx + TW][m]
                over.append(((x.max() - x.min() + 2) | 1) * (y.max() - y.min() + 2) > BUDGET)
    return over


@pytest.mark.parametrize("kind", ["mild", "strong", "zoom"])
@pytest.mark.parametrize("model", ["brown", "fisheye"])
def test_every_calibration_at_every_size(model, kind):
    from codetr import _cabi

    rng, before = np.random.default_rng(len(model) + len(kind)), _cabi.CALLS["undistort"]
    # none the size of its output; the last one large enough for the zoom-out to fill whole tiles
    sources = [(3, 2), (70, 5), (2, 41), (33, 90), (21, 61), (40, 77), (120, 260) if kind == "zoom" else (45, 140)]
    frames = [(rng.integers(0, 256, hw + (3,), dtype=np.uint8), _camera(model, kind, *hw, *size)) for hw, size in zip(sources, SIZES)]
    images = _launch(frames)
    assert _cabi.CALLS["undistort"] == before + 1
    for (im, s), got in zip(frames, images):
        want = R.remap(im, s)
        assert np.array_equal(got, want), (im.shape, s["size"], np.argwhere(got != want)[:4].tolist())
    if kind == "strong":    # part of the largest image is the fill, part is not
        filled = (images[-1] == (200, 30, 90)).all(-1)
        assert filled.any() and not filled.all()
    if kind == "zoom":      # conditions on the inputs, read off the restatement: both paths ran
        over = _over_budget(*frames[-1])
        assert any(over) and not all(over), over
    if kind == "mild":      # ... and here only the staged one
        assert not any(_over_budget(*frames[-1]))


def test_one_launch_mixes_models_and_the_identity_returns_the_input():
    from codetr import hip_ops

    rng = np.random.default_rng(11)
    ims = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in [(33, 90), (40, 77), (35, 131), (120, 260)]]
    frames = [(ims[0], _camera("fisheye", "strong", 33, 90, 19, 70)), (ims[1], _camera("brown", "mild", 40, 77, 50, 66)),
              (ims[2], hip_ops.undistort_settings(dict(camera_matrix=(80.5, 77.25, 60.1, 17.9)), 35, 131)),
              (ims[3], _camera("fisheye", "zoom", 120, 260, 48, 150))]
    images = _launch(frames)
    for (im, s), got in zip(frames, images):
        assert np.array_equal(got, R.remap(im, s)), s["model"]
    assert np.array_equal(images[2], ims[2])


def test_thirty_three_frames_take_two_launches():
    from codetr import _cabi, hip_ops

    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, (9 + k % 5, 20 + k % 7, 3), dtype=np.uint8) for k in range(33)]
    ats = np.cumsum([0] + [im.size for im in ims]).tolist()
    rows = [(im.shape[0], im.shape[1], ats[k], 3 * im.shape[1]) for k, im in enumerate(ims)]
    settings = [_camera(("brown", "fisheye")[k % 2], "mild", *im.shape[:2], *SIZES[3 + k % 3]) for k, im in enumerate(ims)]
    before = _cabi.CALLS["undistort"]
    buf, staged = hip_ops.undistort_frames(torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(DEV), rows, settings)
    assert _cabi.CALLS["undistort"] == before + 2
    host = buf.cpu().numpy()
    for k, (im, s, (off, H, W)) in enumerate(zip(ims, settings, staged)):
        assert off % 16 == 0 and (H, W) == s["size"]
        assert np.array_equal(host[off:off + H * W * 3].reshape(H, W, 3), R.remap(im, s)), k


def _same(out, ref):
    assert [p.pop("undistorted") for p in out["predictions"]] == [True] * len(ref["predictions"])
    assert out["predictions"] == ref["predictions"] and len(out["visualization"]) == len(ref["visualization"])
    assert all(np.array_equal(a, b) for a, b in zip(out["visualization"], ref["visualization"]))


@pytest.mark.parametrize("path", ["plain", "tta", "sliced"])
def test_inferencer_equals_the_call_on_rectified_rgb_arrays(path):
    """NV12 host frames and GPU-resident BGR frames under one calibration dict; then a list of two calibrations with a
    size of their own; then the lens with orientation=6: rectified, then turned"""
    from codetr import _cabi

    nv12 = _items("nv12", 21)
    rgb = [FR.to_rgb(it, "nv12") for it in nv12]
    one = dict(model="fisheye", camera_matrix=(90.0, 88.0, 70.0, 50.0), dist_coeffs=(-0.05, 0.01, 0.0, 0.0), fill=(10, 120, 240))
    rect = [R.remap(a, _settings(one, a)) for a in rgb]
    before = _cabi.CALLS["undistort"]
    ref = _inferencer(**PATHS[path])(rect, **CALL)
    assert _cabi.CALLS["undistort"] == before and not any("undistorted" in p for p in ref["predictions"])   # None: no launch, no key
    _same(_inferencer(**PATHS[path])(nv12, input_format="nv12", undistort=one, **CALL), ref)
    assert _cabi.CALLS["undistort"] == before + 2               # chunks of 3: (3, 2)
    resident = [torch.from_numpy(np.ascontiguousarray(a[..., ::-1])).to(DEV) for a in rgb]
    _same(_inferencer(**PATHS[path])(resident, input_format="bgr", undistort=one, **CALL), ref)
    two = [one, dict(camera_matrix=(120.0, 120.0, 66.0, 41.0), dist_coeffs=(-0.2, 0.05, 0.001, 0.002), new_camera_matrix=(60.0, 60.0, 50.0, 40.0), size=(83, 101))]
    mixed = [two[k % 2] for k in range(len(rgb))]
    out = _inferencer(**PATHS[path])(rgb, undistort=mixed, **CALL)
    _same(out, _inferencer(**PATHS[path])([R.remap(a, _settings(u, a)) for u, a in zip(mixed, rgb)], **CALL))
    turned = _inferencer(**PATHS[path])(nv12, input_format="nv12", undistort=one, orientation=6, **CALL)
    assert [p.pop("orientation") for p in turned["predictions"]] == [6] * len(rgb)
    _same(turned, _inferencer(**PATHS[path])([np.ascontiguousarray(TABLE[6](a)) for a in rect], **CALL))


def _settings(u, image):
    from codetr import hip_ops

    return hip_ops.undistort_settings(u, *image.shape[:2])
