"""GPU: codetr_orient_rgb_u8 (csrc/orient.hip), hip_ops.orient_frames / decode_jpeg and `Inferencer(...)(..., orientation=...)`
byte for byte against the table of test_orient_cpu.py (bytes are only moved: no tolerance).  The files are the committed
ones of tests/golden/orient, decoded by the restatement tests/jpeg_dec_ref.py."""
import numpy as np
import pytest
import torch

import frames_ref as R
import jpeg_dec_ref as D
from test_inferencer_batch_gpu import DEV
from test_jpeg_gpu import PATHS, _inferencer, _items
from test_orient_cpu import NAMES, TABLE, data, expected

pytestmark = pytest.mark.gpu
GUARD = 48
# the tile is 64 x 64: a pixel, a row, a column, one below / at / above the tile, ragged tiles on both axes
SIZES = [(1, 1), (1, 67), (67, 1), (63, 65), (64, 64), (65, 130)]
CALL = dict(batch_size=3, pred_score_thr=0.4, device=DEV, dtype=torch.float16, return_vis=True)


def _launch(frames, seed=3):
    """frames [(o, image)] at odd offsets with pitches 3 W + {0, 1, 5} and random bytes between, one call of the entry point
    into slots at both residues (a multiple of 4, and not) with 0xA5 guard bytes around them -> the upright images"""
    from codetr import _orient

    rows, at, dst = [], 1, GUARD
    for k, (o, im) in enumerate(frames):
        H, W = im.shape[:2]
        dst += (k % 2 - dst) % 4            # even frames at a multiple of 4, odd ones one byte behind it
        rows.append((o, H, W, at, 3 * W + (0, 1, 5)[k % 3], dst))
        at += H * rows[-1][4] + 2
        at += 1 - at % 2                    # (every offset odd)
        dst += H * W * 3 + GUARD
    src = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)
    for (o, H, W, off, pitch, _), (_, im) in zip(rows, frames):
        for y in range(H):
            src[off + y * pitch:off + y * pitch + 3 * W] = im[y].reshape(-1)
    dev = torch.from_numpy(src).to(DEV)
    out = torch.full((dst,), 0xA5, dtype=torch.uint8, device=DEV)
    _orient.orient(dev, rows, out)
    host, images = out.cpu().numpy(), []
    assert np.array_equal(dev.cpu().numpy(), src)          # the stored images are only read
    for o, H, W, _, _, d in rows:
        images.append(host[d:d + H * W * 3].reshape((W, H, 3) if o >= 5 else (H, W, 3)).copy())
        host[d:d + H * W * 3] = 0xA5
    assert (host == 0xA5).all(), "guard bytes around an image were written"
    return images


@pytest.mark.parametrize("o", range(1, 9))
def test_every_orientation_at_every_size(o):
    from codetr import _cabi

    rng, before = np.random.default_rng(10 + o), _cabi.CALLS["orient"]
    frames = [(o, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) for H, W in SIZES]
    images = _launch(frames)
    assert _cabi.CALLS["orient"] == before + 1
    for (_, im), got in zip(frames, images):
        assert np.array_equal(got, TABLE[o](im)), im.shape


def test_thirty_three_mixed_frames_take_two_launches():
    from codetr import _cabi, hip_ops

    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, SIZES[k % 6] + (3,), dtype=np.uint8) for k in range(33)]
    ats = np.cumsum([0] + [im.size for im in ims]).tolist()
    rows = [(1 + k % 8, im.shape[0], im.shape[1], ats[k], 3 * im.shape[1]) for k, im in enumerate(ims)]
    before = _cabi.CALLS["orient"]
    buf, staged = hip_ops.orient_frames(torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(DEV), rows)
    assert _cabi.CALLS["orient"] == before + 2
    host = buf.cpu().numpy()
    for k, (im, (off, H, W)) in enumerate(zip(ims, staged)):
        assert off % 16 == 0 and (H, W) == hip_ops.oriented_size(1 + k % 8, *im.shape[:2])
        assert np.array_equal(host[off:off + H * W * 3].reshape(H, W, 3), TABLE[1 + k % 8](im)), k


def _same(out, ref, orientations):
    assert [p.pop("orientation") for p in out["predictions"]] == list(orientations)
    assert out["predictions"] == ref["predictions"] and len(out["visualization"]) == len(ref["visualization"]) == len(orientations)
    assert all(np.array_equal(a, b) for a, b in zip(out["visualization"], ref["visualization"]))


def test_inferencer_honours_the_exif_tag_of_jpeg_files():
    from codetr import _cabi, hip_ops

    files = [data(n) for n in NAMES]
    stored = [D.decode(f)[0] for f in files]
    upright = [np.ascontiguousarray(TABLE[expected(n)](a)) for n, a in zip(NAMES, stored)]
    before = _cabi.CALLS["orient"]
    out = _inferencer()(files, input_format="jpeg", orientation="exif", **CALL)
    turned_chunks = sum(any(expected(n) != 1 for n in NAMES[i:i + 3]) for i in range(0, len(NAMES), 3))
    assert _cabi.CALLS["orient"] == before + turned_chunks == before + 4   # one launch per chunk of 3; none for (1, 1, 1)
    _same(out, _inferencer()(upright, input_format="rgb", **CALL), [expected(n) for n in NAMES])
    # orientation=None: what the call gave before there was the keyword -- no launch, no key, the stored images
    out = _inferencer()(files, input_format="jpeg", **CALL)
    assert _cabi.CALLS["orient"] == before + 4 and not any("orientation" in p for p in out["predictions"])
    ref = _inferencer()(stored, input_format="rgb", **CALL)
    assert out["predictions"] == ref["predictions"] and all(np.array_equal(a, b) for a, b in zip(out["visualization"], ref["visualization"]))
    buf, staged = hip_ops.decode_jpeg(files, device=DEV, orientation="exif")   # the same images without the Inferencer
    for (off, H, W), exp in zip(staged, upright):
        assert off % 16 == 0 and np.array_equal(buf.cpu().numpy()[off:off + H * W * 3].reshape(H, W, 3), exp)
    with pytest.raises(ValueError, match="input_format"):
        _inferencer()(stored, orientation="exif", **CALL)
    x, _, metas = _inferencer().preprocess_batch(files, DEV, torch.float16, input_format="jpeg", orientation="exif")
    xr, _, metas_r = _inferencer().preprocess_batch(upright, DEV, torch.float16)
    assert torch.equal(x, xr) and metas == metas_r


@pytest.mark.parametrize("path", ["plain", "tta", "sliced"])
def test_turned_frames_equal_the_turned_rgb_arrays(path):
    """NV12 host frames and GPU-resident BGR frames under one orientation, then host RGB arrays with one each: an o = 1
    frame between a 6 and a 3, and a chunk of 1s that launches nothing; the TTA and slicing tails see the upright sizes"""
    from codetr import _cabi

    nv12 = _items("nv12", 21)
    rgb = [R.to_rgb(it, "nv12") for it in nv12]
    ref = _inferencer(**PATHS[path])([np.ascontiguousarray(TABLE[6](a)) for a in rgb], **CALL)
    _same(_inferencer(**PATHS[path])(nv12, input_format="nv12", orientation=6, **CALL), ref, [6] * len(nv12))
    resident = [torch.from_numpy(np.ascontiguousarray(a[..., ::-1])).to(DEV) for a in rgb]
    _same(_inferencer(**PATHS[path])(resident, input_format="bgr", orientation=6, **CALL), ref, [6] * len(nv12))
    mixed, before = [6, 1, 3, 1, 1], _cabi.CALLS["orient"]         # chunks of 3: (6, 1, 3) and (1, 1)
    out = _inferencer(**PATHS[path])(rgb, orientation=mixed, **CALL)
    assert _cabi.CALLS["orient"] == before + 1
    _same(out, _inferencer(**PATHS[path])([np.ascontiguousarray(TABLE[o](a)) for o, a in zip(mixed, rgb)], **CALL), mixed)
