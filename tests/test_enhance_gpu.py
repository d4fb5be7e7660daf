"""GPU: codetr_enhance_rgb_u8 (csrc/enhance.hip), hip_ops.enhance_frames and `Inferencer(...)(..., enhance=...)` byte for
byte against the restatement tests/enhance_ref.py (the rule is exact: no tolerance)."""
import numpy as np
import pytest
import torch

import enhance_ref as R
from test_inferencer_batch_gpu import DEV
from test_jpeg_gpu import PATHS, _inferencer, _items

pytestmark = pytest.mark.gpu
GUARD = 48
CALL = dict(batch_size=3, pred_score_thr=0.4, device=DEV, dtype=torch.float16, return_vis=True)
# (size, grid): a pixel; 1 x 1-pixel tiles; sides the grid does not divide, on y, on x and on both, so that reflected padding
# counts; tiles that lie in the padding alone; widths 13..15, which with the pitches below put every dword phase at a row's
# head and tail; a tile (and a lattice cell's band) just below, at and just above one slice of 8192 samples; a tile so wide
# that the slice count is capped (40 rows of 8200 -> 20 slices of 2 rows)
CASES = [((1, 1), (1, 1)), ((5, 7), (5, 7)), ((37, 64), (4, 8)), ((32, 150), (4, 8)), ((37, 150), (4, 8)), ((9, 9), (8, 8)),
         ((6, 13), (2, 3)), ((6, 14), (2, 3)), ((6, 15), (2, 3)), ((127, 64), (1, 1)), ((128, 64), (1, 1)), ((129, 64), (1, 1)),
         ((40, 8200), (1, 1))]


def _image(content, H, W, rng):
    if content == "constant":      # the worst contention and the largest excess
        return np.broadcast_to(np.uint8([200, 30, 90]), (H, W, 3)).copy()
    if content == "ramp":          # all 256 values where the image has that many pixels
        v = np.arange(H * W).reshape(H, W)
        return np.stack([v, 255 - v, v * 7], -1).astype(np.uint8)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _launch(frames, in_place):
    """frames [(image, grid, clip_limit)] at odd offsets with pitches 3 W + {0, 1, 5} and random bytes between, one call of the
    entry point -- in place, or into slots at both residues (a multiple of 4, and not) with pitches 3 W + {0, 7} and 0xA5
    between and around them -> the enhanced images; no byte outside an image's rows may change"""
    from codetr import _enhance

    rows, at, dst = [], 1, GUARD
    for k, (im, grid, clip) in enumerate(frames):
        H, W = im.shape[:2]
        pitch, dpitch = 3 * W + (0, 1, 5)[k % 3], 3 * W + (0, 7)[k % 2]
        dst += (k % 2 - dst) % 4            # even frames at a multiple of 4, odd ones one byte behind it
        C = R.clip_count(clip, -(-H // grid[0]) * -(-W // grid[1]))
        rows.append((H, W, at, pitch) + ((at, pitch) if in_place else (dst, dpitch)) + tuple(grid) + (C,))
        at += H * pitch + 2
        at += 1 - at % 2                    # (every offset odd)
        dst += H * dpitch + GUARD
    src = np.random.default_rng(3).integers(0, 256, at, dtype=np.uint8)
    for (H, W, off, pitch, *_), (im, _, _) in zip(rows, frames):
        for y in range(H):
            src[off + y * pitch:off + y * pitch + 3 * W] = im[y].reshape(-1)
    dev = torch.from_numpy(src).to(DEV)
    out = dev.clone() if in_place else torch.full((dst,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.empty((_enhance.workspace_bytes(rows) // 4,), dtype=torch.int32, device=DEV)
    _enhance.enhance(out if in_place else dev, rows, out, ws)
    host, images = out.cpu().numpy(), []
    untouched = src.copy() if in_place else np.full(dst, 0xA5, np.uint8)
    for H, W, _, _, d, dp, *_ in rows:
        at = [slice(d + y * dp, d + y * dp + 3 * W) for y in range(H)]
        images.append(np.stack([host[s] for s in at]).reshape(H, W, 3))
        for s in at:
            untouched[s] = host[s]
    assert np.array_equal(host, untouched), "bytes outside the images' rows were written"
    assert np.array_equal(dev.cpu().numpy(), src)          # out of place the stored frames are only read
    return images


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("clip_limit", [None, 1 / 256, 2.0])
@pytest.mark.parametrize("content", ["constant", "ramp", "random"])
def test_every_case_in_one_call(content, clip_limit, in_place):
    from codetr import _cabi

    rng, before = np.random.default_rng(len(content)), _cabi.CALLS["enhance"]
    frames = [(_image(content, H, W, rng), grid, clip_limit) for (H, W), grid in CASES]
    images = _launch(frames, in_place)
    assert _cabi.CALLS["enhance"] == before + 1
    for (im, grid, clip), got in zip(frames, images):
        want = R.enhance(im, grid, clip)
        assert np.array_equal(got, want), (im.shape, grid, np.argwhere(got != want)[:4].tolist())


def test_thirty_three_frames_take_two_calls_and_in_place_wants_packed_rows():
    from codetr import _cabi, hip_ops

    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, (9 + k % 5, 20 + k % 7, 3), dtype=np.uint8) for k in range(33)]
    ats = np.cumsum([0] + [im.size for im in ims]).tolist()
    rows = [(im.shape[0], im.shape[1], ats[k], 3 * im.shape[1]) for k, im in enumerate(ims)]
    settings = [dict(grid=(1 + k % 3, 2 + k % 4), clip_limit=(None, 0.5, 3.0)[k % 3]) for k in range(33)]
    src, before, cache = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(DEV), _cabi.CALLS["enhance"], {}
    buf, staged = hip_ops.enhance_frames(src, rows, settings, workspace=cache)
    assert _cabi.CALLS["enhance"] == before + 2 and list(cache) == [src.device]
    host = buf.cpu().numpy()
    for k, (im, s, (off, H, W)) in enumerate(zip(ims, settings, staged)):
        assert off % 16 == 0 and (H, W) == im.shape[:2]
        assert np.array_equal(host[off:off + H * W * 3].reshape(H, W, 3), R.enhance(im, **s)), k
    same, where = hip_ops.enhance_frames(src, rows, settings, out=src, workspace=cache)
    assert same is src and where == [(at, H, W) for H, W, at, _ in rows] and len(cache) == 1
    assert all(np.array_equal(src[at:at + H * W * 3].cpu().numpy(), host[off:off + H * W * 3]) for (at, H, W), (off, _, _) in zip(where, staged))
    with pytest.raises(ValueError, match="packed"):
        hip_ops.enhance_frames(src, [(9, 19, 0, 60)], {}, out=src)
    with pytest.raises(ValueError, match="more tiles"):
        hip_ops.enhance_frames(src, rows[:1], dict(grid=(10, 2)))


def test_inferencer_equals_the_call_on_enhanced_rgb_arrays():
    """host RGB frames under one dict (the uploaded buffer enhanced in place), GPU-resident BGR frames under a list of two
    (the conversion's output enhanced, the caller's tensors untouched); None launches nothing and adds no key"""
    from codetr import _cabi

    rgb = _items("rgb", 21)
    one, two = dict(grid=(4, 6), clip_limit=3.0), [dict(grid=(2, 2), clip_limit=None), dict()]
    before = _cabi.CALLS["enhance"]
    ref = _inferencer(**PATHS["plain"])([R.enhance(a, **one) for a in rgb], **CALL)
    assert _cabi.CALLS["enhance"] == before and not any("enhanced" in p for p in ref["predictions"])
    for frames, fmt, settings in [(rgb, "rgb", one), ([torch.from_numpy(np.ascontiguousarray(a[..., ::-1])).to(DEV) for a in rgb], "bgr", None)]:
        per_image = settings or [two[k % 2] for k in range(len(rgb))]
        if settings is None:
            ref = _inferencer(**PATHS["plain"])([R.enhance(a, **{**dict(grid=(8, 8), clip_limit=2.0), **s}) for a, s in zip(rgb, per_image)], **CALL)
        before = _cabi.CALLS["enhance"]
        out = _inferencer(**PATHS["plain"])(frames, input_format=fmt, enhance=per_image, **CALL)
        assert _cabi.CALLS["enhance"] == before + 2               # chunks of 3: (3, 2)
        assert [p.pop("enhanced") for p in out["predictions"]] == [True] * len(rgb)
        assert out["predictions"] == ref["predictions"] and len(out["visualization"]) == len(rgb)
        assert all(np.array_equal(a, b) for a, b in zip(out["visualization"], ref["visualization"]))
        if fmt == "bgr":
            assert all(np.array_equal(t.cpu().numpy()[..., ::-1], a) for t, a in zip(frames, rgb))
