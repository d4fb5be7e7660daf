"""GPU: codetr_raw_to_rgb_u8 (csrc/raw.hip), hip_ops.raw_to_rgb and `Inferencer(...)(..., input_format="bayer_*", raw=...)`
byte for byte against the restatement tests/raw_ref.py (the rule is exact integers: no tolerance)."""
import numpy as np
import pytest
import torch

import raw_ref as R
from test_inferencer_batch_gpu import DEV
from test_jpeg_gpu import _inferencer, _smooth

pytestmark = pytest.mark.gpu
GUARD = 48
# the tile is 64 x 64 with a halo of 2: a pixel, a row, a column (every halo sample folded, some twice), the smallest
# period, an odd one, one below / at / above the tile, ragged tiles on both axes
SIZES = [(1, 1), (1, 67), (67, 1), (2, 2), (3, 5), (63, 65), (64, 64), (65, 130)]
CALL = dict(batch_size=2, pred_score_thr=0.4, device=DEV, dtype=torch.float16, return_vis=True)


def _launch(frames, pattern, raw, seed=3):
    """frames [H, W] (uint8: at odd offsets, pitches W + {0, 1, 5}; uint16: even offsets, 2 W + {0, 2, 6}), random bytes
    between, one call into slots at both residues mod 4 with 0xA5 guard bytes around them -> the images"""
    from codetr import _raw, hip_ops

    s = hip_ops.raw_settings(raw)
    B = frames[0].itemsize
    rows, at, dst = [], 2 - B, GUARD
    for k, im in enumerate(frames):
        H, W = im.shape
        dst += (k % 2 - dst) % 4            # even frames at a multiple of 4, odd ones one byte behind it
        rows.append((R.PATTERNS[pattern], s["bits"], H, W, at, B * W + ((0, 1, 5), (0, 2, 6))[B - 1][k % 3], dst))
        at += H * rows[-1][5] + 2
        at += (2 - B - at) % 2              # (8-bit: every offset odd; 16-bit: even)
        dst += H * W * 3 + GUARD
    src = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)
    for (_, _, H, W, off, pitch, _), im in zip(rows, frames):
        for y in range(H):
            src[off + y * pitch:off + y * pitch + B * W] = im[y].view(np.uint8)
    dev = torch.from_numpy(src).to(DEV)
    out = torch.full((dst,), 0xA5, dtype=torch.uint8, device=DEV)
    _raw.to_rgb(dev, rows, s["operands"], torch.from_numpy(s["lut"]).to(DEV), out)
    host, images = out.cpu().numpy(), []
    assert np.array_equal(dev.cpu().numpy(), src)          # the frames are only read
    for _, _, H, W, _, _, d in rows:
        images.append(host[d:d + H * W * 3].reshape(H, W, 3).copy())
        host[d:d + H * W * 3] = 0xA5
    assert (host == 0xA5).all(), "guard bytes around an image were written"
    return images, s


def _frames(bits, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2 ** bits, size, dtype=np.uint8 if bits == 8 else np.uint16) for size in SIZES]


def _same_as_rule(frames, images, pattern, s):
    kw = {k: s[k] for k in ("bits", "black_level", "white_level", "white_balance", "method")}
    for im, got in zip(frames, images):
        assert np.array_equal(got, R.demosaic(im, pattern, lut=s["lut"], **kw)), im.shape


LEVELS = dict(bits=12, black_level=240, white_level=3800, white_balance=(2.1, 1.0, 1.6), tone="srgb")
CASES = [(p, dict(bits=b, method=m)) for m in ("malvar", "bilinear") for p in sorted(R.PATTERNS) for b in (8, 12)] + [("bayer_gbrg", LEVELS)]


@pytest.mark.parametrize("pattern,raw", CASES, ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v.values()))
def test_every_pattern_and_method_at_every_size(pattern, raw):
    from codetr import _cabi

    frames, before = _frames(raw["bits"], 10 + raw["bits"] + R.PATTERNS[pattern]), _cabi.CALLS["raw"]
    images, s = _launch(frames, pattern, raw)
    assert _cabi.CALLS["raw"] == before + 1
    _same_as_rule(frames, images, pattern, s)


def test_thirty_three_frames_take_two_launches():
    from codetr import _cabi, hip_ops

    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, SIZES[k % 8], dtype=np.uint8) for k in range(33)]
    ats = np.cumsum([0] + [im.size for im in ims]).tolist()
    dsts = np.cumsum([0] + [-(-im.size * 3 // 16) * 16 for im in ims]).tolist()
    rows = [("bayer_bggr", 8, im.shape[0], im.shape[1], ats[k], im.shape[1], dsts[k]) for k, im in enumerate(ims)]
    before = _cabi.CALLS["raw"]
    buf = hip_ops.raw_to_rgb(torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(DEV), rows, dsts[-1])
    assert _cabi.CALLS["raw"] == before + 2
    host = buf.cpu().numpy()
    for k, im in enumerate(ims):
        assert np.array_equal(host[dsts[k]:dsts[k] + im.size * 3].reshape(im.shape + (3,)), R.demosaic(im, "bayer_bggr")), k


def test_inferencer_takes_raw_frames_from_the_host_and_resident():
    """one scene as 12-bit mosaics from the host, as GPU-resident pitched uint16 views (turned by orientation=6), and as the
    restatement's RGB arrays: the same predictions and the same drawn images"""
    from codetr import _cabi, hip_ops

    rng, raw = np.random.default_rng(21), dict(bits=12, white_balance=(1.8, 1.0, 1.5), tone="srgb")
    mosaics = [(_smooth(size, rng).astype(np.uint16) * 16 + 7) for size in [(120, 160), (97, 131), (64, 200)]]
    s = hip_ops.raw_settings(raw)
    rgb = [R.demosaic(m, "bayer_rggb", bits=12, white_balance=raw["white_balance"], lut=s["lut"]) for m in mosaics]
    wide = [torch.from_numpy(np.pad(m, ((0, 0), (1, 2))).view(np.int16)).to(DEV) for m in mosaics]   # a wider surface
    resident = [w.view(torch.uint16)[:, 1:1 + m.shape[1]] for w, m in zip(wide, mosaics)]
    before = _cabi.CALLS["raw"]
    for frames, kw in ((mosaics, {}), (resident, dict(orientation=6))):
        out = _inferencer()(frames, input_format="bayer_rggb", raw=raw, **kw, **CALL)
        ref = _inferencer()(rgb, input_format="rgb", **kw, **CALL)
        assert out["predictions"] == ref["predictions"] and len(out["visualization"]) == 3
        assert all(np.array_equal(a, b) for a, b in zip(out["visualization"], ref["visualization"]))
    assert _cabi.CALLS["raw"] == before + 2 + 3             # host: chunks of 2 and 1; resident: one launch per storage
    with pytest.raises(ValueError, match="even"):
        _inferencer()([w.view(torch.uint8)[:, 1:9] for w in wide], input_format="bayer_rggb", raw=raw, **CALL)
