"""GPU: codetr_frames_to_rgb_u8 (csrc/frames.hip) against the numpy restatement of its header text (tests/frames_ref.py),
bit-equal over whole output buffers -- the sentinel bytes between and behind the images included --, and
`Inferencer(...)(frames, input_format=...)` against the same call on the reference's RGB conversion of those frames."""
import numpy as np
import pytest
import torch

import frames_ref as R
from test_inferencer_batch_gpu import DEV, SWIN, _images, _same
from test_tta_gpu import _stub

pytestmark = pytest.mark.gpu
COMBOS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
# odd sides, a row tail in every position mod 4 (1, 2, 5 -> 1, 257 -> 1, 66 -> 2, 1028 -> 0 with 3 and 7 below), a row
# longer than one 256-thread workgroup of 4-pixel groups (1028 > 1024)
SIZES = [(1, 1), (2, 2), (3, 5), (7, 257), (64, 66), (33, 1028)]
SENTINEL = 0x5A


def _convert(frames, matrix="bt601", range_="limited", **layout):
    """pack the frames, run the kernel into a sentinel-filled buffer a few bytes longer than needed, compare every byte"""
    from codetr import hip_ops

    buf, rows, dst_bytes = R.pack(frames, **layout)
    total = dst_bytes + 5
    out = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    got = hip_ops.frames_to_rgb(torch.from_numpy(buf).to(DEV), rows, total, matrix, range_, out=out)
    assert got is out
    got = out.cpu().numpy()
    expect = R.expected_output(frames, rows, total, SENTINEL, matrix, range_)
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), expect[bad[:8]].tolist(), rows)
    return got


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_every_format_matrix_and_range_at_every_size(fmt):
    rng = np.random.default_rng(R.FORMATS[fmt])
    frames = [(fmt, H, W, R.random_planes(fmt, H, W, rng)) for H, W in SIZES + [(5, 3), (2, 7)]]
    for matrix, range_ in COMBOS:
        _convert(frames, matrix, range_)                       # rows packed, everything 4-byte aligned where it can be
    _convert(frames, "bt709", "full", start=1, dst_start=2)    # ... and from odd addresses on both sides


@pytest.mark.parametrize("matrix,range_", COMBOS)
def test_exhaustive_arithmetic(matrix, range_):
    """one I420 frame in which every (Y, U) pair meets every V of the list: chroma sample (cy, cx) holds U = cx and
    V = VS[cy // 64]; the four pixels under it hold Y = 4 * (cy % 64) + 0..3"""
    VS = np.array([0, 1, 15, 16, 17, 127, 128, 129, 239, 240, 241, 254, 255], np.uint8)
    ch, cw = 64 * len(VS), 256
    U = np.broadcast_to(np.arange(cw, dtype=np.uint8)[None, :], (ch, cw)).copy()
    V = np.broadcast_to(np.repeat(VS, 64)[:, None], (ch, cw)).copy()
    yy, xx = np.arange(2 * ch)[:, None], np.arange(2 * cw)[None, :]
    Y = (4 * ((yy >> 1) % 64) + 2 * (yy & 1) + (xx & 1)).astype(np.uint8)
    pairs = Y[:128].astype(np.int64) * 256 + U[(yy >> 1), (xx >> 1)][:128]        # the rows of one V
    assert np.unique(pairs).size == 65536 and np.unique(V[::64, 0]).size == len(VS)
    _convert([("i420", 2 * ch, 2 * cw, [Y, U, V])], matrix, range_)


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_pitched_planes_ignore_what_lies_between_the_rows(fmt):
    rng = np.random.default_rng(20 + R.FORMATS[fmt])
    frames = [(fmt, H, W, R.random_planes(fmt, H, W, rng)) for H, W in ((7, 257), (5, 12), (3, 5), (64, 66))]
    outs = [_convert(frames, "bt601", "full", pad=pad, fill=fill) for pad in (1, 6, 8) for fill in (0x00, 0xA5)]
    for a, b in zip(outs[::2], outs[1::2]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_offsets_at_every_residue_and_mixed_formats_in_one_launch(shift):
    """every format at two sizes in one launch (16 frames): consecutive planes start at consecutive residues mod 4, so
    over the four shifts every plane of every frame sees all of them; the outputs likewise.  W = 12 keeps whole 4-pixel
    groups -- the dword paths, where the address allows -- and W = 7 a tail."""
    from codetr import _cabi

    rng = np.random.default_rng(40 + shift)
    frames = [(fmt, H, W, R.random_planes(fmt, H, W, rng)) for fmt in R.FORMATS for H, W in ((5, 12), (3, 7))]
    before = _cabi.CALLS["frames_to_rgb"]
    _convert(frames, "bt709", "limited", start=shift, residues=[shift, (shift + 1) % 4, (shift + 2) % 4, (shift + 3) % 4],
             dst_residues=[shift, (shift + 3) % 4, (shift + 2) % 4, (shift + 1) % 4], dst_start=shift, pad=shift)
    assert _cabi.CALLS["frames_to_rgb"] == before + 1


def test_the_last_plane_may_end_flush_with_the_source_buffer():
    """R.pack ends the buffer with the last row of the last plane; a pitched one-plane and a three-plane frame, odd sizes"""
    from codetr import _cabi

    rng = np.random.default_rng(50)
    for fmt in ("gray", "rgba", "nv21", "i420"):
        frames = [(fmt, 3, 5, R.random_planes(fmt, 3, 5, rng))]
        buf, rows, _ = R.pack(frames, pad=3, start=2)
        k = len(frames[0][3]) - 1
        rb = frames[0][3][k].shape[1]
        assert rows[0][3 + 2 * k] + (frames[0][3][k].shape[0] - 1) * (rb + 3) + rb == buf.size
        _convert(frames, pad=3, start=2)
        with pytest.raises(RuntimeError, match="codetr_frames_to_rgb_u8"):       # one byte less: rejected, not read
            _cabi.frames_to_rgb(torch.from_numpy(buf[:-1].copy()).to(DEV), rows, 0, 0,
                                torch.empty((1024,), dtype=torch.uint8, device=DEV))


def test_33_frames_split_into_two_launches():
    from codetr import _cabi

    rng = np.random.default_rng(60)
    fmts = list(R.FORMATS)
    frames = [(fmts[i % 8], 3 + i % 5, 4 + i % 7, None) for i in range(33)]
    frames = [(f, H, W, R.random_planes(f, H, W, rng)) for f, H, W, _ in frames]
    before = _cabi.CALLS["frames_to_rgb"]
    _convert(frames, "bt601", "limited", pad=1, dst_residues=[0, 1, 2, 3])
    assert _cabi.CALLS["frames_to_rgb"] == before + 2


def test_hip_ops_frames_to_rgb_checks_its_arguments():
    from codetr import hip_ops

    src = torch.zeros((64,), dtype=torch.uint8, device=DEV)
    row = ("gray", 2, 2, 0, 2, 0, 0, 0, 0, 0)
    out = hip_ops.frames_to_rgb(src, [row], 12)
    assert out.shape == (12,) and out.device == src.device and int(out.sum()) == 0
    with pytest.raises(RuntimeError, match="MI355X"):
        hip_ops.frames_to_rgb(src.cpu(), [row], 12)
    for bad, kw in (([("yuyv",) + row[1:]], {}), ([row[:9]], {}), ([row], dict(matrix="bt2020")), ([row], dict(range="tv")),
                    ([], {}), ([row], dict(out=torch.zeros((11,), dtype=torch.uint8, device=DEV)))):
        with pytest.raises(ValueError, match="frames_to_rgb"):
            hip_ops.frames_to_rgb(src, bad, 12, **kw)
    with pytest.raises(RuntimeError, match="codetr_frames_to_rgb_u8"):            # the entry point's own checks
        hip_ops.frames_to_rgb(src, [row], 11)


# ---- the Inferencer ----------------------------------------------------------------------------------------------
FRAME_SIZES = [(480, 640), (37, 53), (300, 1000), (128, 96), (600, 900)]       # 37 x 53: odd, so a tuple of planes
PATHS = {
    "plain": dict(),
    "soft": dict(nms_type="config"),
    "tta": dict(tta=dict(scales=[(320, 200), (400, 256)], flip=True, max_per_img=50)),
    "sliced": dict(slicing=dict(tile=(300, 200), tile_batch=8, max_per_img=100)),
}


def _frames(fmt, seed):
    """the chunk items of one format and the RGB images the reference makes of them"""
    rng = np.random.default_rng(seed)
    if fmt == "bgr":
        items = [im[..., ::-1] for im in _images(FRAME_SIZES, seed)]            # (host views with a negative stride)
    else:
        items = [R.item(fmt, H, W, R.random_planes(fmt, H, W, rng)) for H, W in FRAME_SIZES]
    return items, [R.to_rgb(it, fmt) for it in items]


def _inferencer(model, **kw):
    from codetr.inferencer import Inferencer

    inf = Inferencer(model, SWIN, dataset_meta=None, score_threshold=0.3, visualizer=dict(), **kw)
    inf.scale = (400, 256)          # (small inputs: the shipped scale would make every tile a 768 x 768 image)
    inf.pad_size = None             # (no fixed Pad: the stub reads the middle row of the batch, which must hold pixels)
    return inf


def _equal_results(a, b):
    _same(a["predictions"], b["predictions"])
    assert len(a["visualization"]) == len(b["visualization"]) == len(a["predictions"])
    for x, y in zip(a["visualization"], b["visualization"]):
        assert x.dtype == np.uint8 and x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("path", list(PATHS))
def test_inferencer_on_frames_equals_the_call_on_their_rgb_conversion(path, dtype):
    from codetr import _cabi

    inf = _inferencer(_stub([]), **PATHS[path])
    for fmt in ("nv12", "i420", "bgr"):
        items, rgb = _frames(fmt, 70 + R.FORMATS[fmt])
        before = dict(_cabi.CALLS)
        got = inf(items, input_format=fmt, batch_size=4, return_vis=True, device=DEV, dtype=dtype)
        assert _cabi.CALLS["frames_to_rgb"] - before["frames_to_rgb"] == 2      # one launch per chunk
        assert _cabi.CALLS["preprocess"] == before["preprocess"]               # never the per-image path
        before = dict(_cabi.CALLS)
        expect = inf(rgb, batch_size=4, return_vis=True, device=DEV, dtype=dtype)
        assert _cabi.CALLS["frames_to_rgb"] == before["frames_to_rgb"]
        _equal_results(got, expect)
        assert sum(len(p["labels"]) for p in got["predictions"]) > 0
        if path == "plain":        # undrawn: the converted frames come back, not the caller's arrays
            undrawn = inf(items, input_format=fmt, batch_size=4, return_vis=True, draw_pred=False, device=DEV, dtype=dtype)
            assert all(np.array_equal(a, b) for a, b in zip(undrawn["visualization"], rgb))
            # ... and at batch_size 1 a frame still takes the chunked path
            one = inf(items[:2], input_format=fmt, device=DEV, dtype=dtype)
            _same(one["predictions"], inf(rgb[:2], device=DEV, dtype=dtype, batch_size=1)["predictions"])
            assert _cabi.CALLS["preprocess"] == before["preprocess"] + (2 if dtype != torch.bfloat16 else 0)


def test_other_matrix_and_range_reach_the_kernel():
    inf = _inferencer(_stub([]))
    items, _ = _frames("nv12", 80)
    color = dict(matrix="bt709", range="full")
    got = inf(items, input_format="nv12", color=color, batch_size=4, return_vis=True, draw_pred=False, device=DEV,
              dtype=torch.float16)
    for vis, it in zip(got["visualization"], items):
        assert np.array_equal(vis, R.to_rgb(it, "nv12", "bt709", "full"))
    expect = inf([R.to_rgb(it, "nv12", "bt709", "full") for it in items], batch_size=4, device=DEV, dtype=torch.float16)
    _same(got["predictions"], expect["predictions"])


def _surface(fmt, H, W, rng, pitch, top=3, left=8):
    """one decoder-style surface [rows, pitch] of random bytes on the GPU and the frame at (top, left) in it as views:
    -> (the item of GPU views, the same frame as host arrays)"""
    rows = {"nv12": H + (H + 1) // 2, "i420": H + 2 * ((H + 1) // 2), "rgb": H, "gray": H}[fmt]
    host = rng.integers(0, 256, (top + rows, pitch), dtype=np.uint8)
    dev = torch.from_numpy(host).to(DEV)
    ch, cw = (H + 1) // 2, (W + 1) // 2

    def views(a):
        body = a[top:]
        if fmt == "nv12":
            uv = body[H:H + ch, left:left + 2 * cw]
            return body[:H, left:left + W], uv.reshape(ch, cw, 2) if isinstance(uv, np.ndarray) else uv.unflatten(1, (cw, 2))
        if fmt == "i420":
            return body[:H, left:left + W], body[H:H + ch, left:left + cw], body[H + ch:H + 2 * ch, left:left + cw]
        if fmt == "gray":
            return body[:H, left:left + W]
        px = body[:H, left:left + 3 * W]
        return px.reshape(H, W, 3) if isinstance(px, np.ndarray) else px.unflatten(1, (W, 3))

    return views(dev), views(host)


@pytest.mark.parametrize("path,dtype", [("plain", torch.float16), ("tta", torch.bfloat16), ("sliced", torch.float16)])
def test_gpu_resident_frames_equal_the_same_frames_from_the_host(path, dtype):
    from codetr import _cabi

    rng = np.random.default_rng(90)
    inf = _inferencer(_stub([]), **PATHS[path])
    for fmt in ("nv12", "i420", "rgb"):
        pairs = [_surface(fmt, H, W, rng, pitch * (3 if fmt == "rgb" else 1))
                 for (H, W), pitch in zip(FRAME_SIZES, (704, 256, 3072, 128, 2816))]
        on_gpu, on_host = [p[0] for p in pairs], [p[1] for p in pairs]
        if fmt == "nv12":   # the 2-D array of a decoder, unpitched, already on the GPU
            flat = R.item("nv12", 128, 96, R.random_planes("nv12", 128, 96, rng))
            on_gpu[3], on_host[3] = torch.from_numpy(flat).to(DEV), flat
        if fmt == "rgb":    # host arrays for the reference; host tensors take the staged route too
            on_host = [np.ascontiguousarray(a) for a in on_host]
        before = dict(_cabi.CALLS)
        got = inf(on_gpu, input_format=fmt, batch_size=4, return_vis=True, device=DEV, dtype=dtype)
        # every frame has a storage of its own: one launch each
        assert _cabi.CALLS["frames_to_rgb"] - before["frames_to_rgb"] == 5
        expect = inf(on_host, input_format=fmt, batch_size=4, return_vis=True, device=DEV, dtype=dtype)
        _equal_results(got, expect)
        mixed = [g if i % 2 else h for i, (g, h) in enumerate(zip(on_gpu, on_host))]
        if fmt != "rgb":
            _equal_results(inf(mixed, input_format=fmt, batch_size=4, return_vis=True, device=DEV, dtype=dtype), expect)
    # two frames cut from one surface share a launch
    host = rng.integers(0, 256, (200, 512), dtype=np.uint8)
    dev = torch.from_numpy(host).to(DEV)

    def cut(a):
        return [a[:96, :128], a[100:196, 256:384]]

    before = _cabi.CALLS["frames_to_rgb"]
    got = inf(cut(dev), input_format="gray", batch_size=2, device=DEV, dtype=dtype)
    assert _cabi.CALLS["frames_to_rgb"] == before + 1
    _same(got["predictions"], inf(cut(host), input_format="gray", batch_size=2, device=DEV, dtype=dtype)["predictions"])


def test_gpu_resident_rejections():
    from codetr.inferencer import parse_frame

    t = torch.zeros((12, 16), dtype=torch.uint8, device=DEV)
    fr = parse_frame(t[:6, 2:6], "nv12")
    assert fr.resident and [tuple(p.stride()) for p in fr.planes] == [(16, 1), (16, 1)]
    assert [p.storage_offset() for p in fr.planes] == [2, 66]
    with pytest.raises(ValueError, match="input_format='gray'.*unit innermost stride"):
        parse_frame(t[:, ::2], "gray")
    with pytest.raises(ValueError, match="input_format='gray'.*unit innermost stride"):
        parse_frame(t[:4, :4].t(), "gray")
    with pytest.raises(ValueError, match="input_format='rgb'.*unit innermost stride"):
        parse_frame(torch.zeros((3, 4, 5), dtype=torch.uint8, device=DEV).permute(1, 2, 0), "rgb")
    with pytest.raises(ValueError, match="input_format='i420'.*must be contiguous"):
        parse_frame(t[:6, :8], "i420")
    with pytest.raises(ValueError, match="input_format='nv12'.*share one storage"):
        parse_frame((t[:4, :6], torch.zeros((2, 3, 2), dtype=torch.uint8, device=DEV)), "nv12")
    with pytest.raises(ValueError, match="input_format='nv12'.*share one storage"):
        parse_frame((t[:4, :6], np.zeros((2, 3, 2), np.uint8)), "nv12")


def _parent_chunk(inf, images, dtype):
    """the chunked path as it was before frames: the images back to back, one upload, one preprocess_batch launch"""
    from codetr import hip_ops
    from codetr.inferencer import rescale_size

    rows, offset = [], 0
    for im in images:
        H, W = im.shape[:2]
        nh, nw = rescale_size(H, W, inf.scale)
        Wp, Hp = (max(inf.pad_size[0], nw), max(inf.pad_size[1], nh)) if inf.pad_size is not None else (nw, nh)
        rows.append((offset, H, W, nh, nw, Hp, Wp))
        offset += im.size
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    return hip_ops.preprocess_batch(src, rows, (max(r[5] for r in rows), max(r[6] for r in rows)), inf.mean, inf.std,
                                    inf.pad_val, inf.pad_value, dtype), rows


def test_rgb_host_arrays_take_the_path_they_took():
    from codetr import _cabi
    from codetr.inferencer import Inferencer

    seen = []
    inf = Inferencer(_stub(seen), SWIN, dataset_meta=None, score_threshold=0.3)
    inf.scale, inf.pad_size = (400, 256), None     # (the stub reads the middle row of the batch: keep pixels there)
    assert inf.pad_size_divisor == 1
    images = _images([(480, 640), (37, 53), (300, 1000)], 95)
    before = dict(_cabi.CALLS)
    x, m, metas, src, staged = inf._preprocess_chunk(images, DEV, torch.float16)
    (px, pm), rows = _parent_chunk(inf, images, torch.float16)
    assert staged == [r[:3] for r in rows]                                 # packed back to back, as before
    assert np.array_equal(src.cpu().numpy(), np.concatenate([im.reshape(-1) for im in images]))
    assert torch.equal(x.view(torch.int16), px.view(torch.int16)) and torch.equal(m, pm)
    got = inf(images, device=DEV, dtype=torch.float16, batch_size=2, input_format="rgb")["predictions"]
    expect = []
    for chunk in (images[:2], images[2:]):
        (px, pm), rows = _parent_chunk(inf, chunk, torch.float16)
        metas = [dict(scale_factor=(r[4] / r[2], r[3] / r[1])) for r in rows]
        expect += inf.postprocess_batch(inf.model(px, pm), metas)
    _same(got, expect)
    assert sum(len(p["labels"]) for p in got) > 0
    one = inf(images, device=DEV, dtype=torch.float16)["predictions"]      # batch_size 1: the per-image path, as before
    assert _cabi.CALLS["preprocess"] == before["preprocess"] + 3
    assert _cabi.CALLS["frames_to_rgb"] == before["frames_to_rgb"] and len(one) == 3


def test_frames_with_the_tiny_model():
    import codetr
    from codetr import _cabi
    from codetr.inferencer import Inferencer
    from helpers_model import seeded_params
    from test_model_gpu import _tiny_codetr_cfg

    dtype = torch.float16
    torch.manual_seed(0)
    model = codetr.CoDETR(**_tiny_codetr_cfg("swin"))
    spec = [(k, tuple(v.shape)) for k, v in model.named_parameters()]
    full = dict(model.state_dict())
    full.update(seeded_params(spec, 77, scale=1.5))
    model.load_state_dict(full)
    model = model.to(DEV, dtype).eval()
    inf = Inferencer(model, SWIN, dataset_meta=None, visualizer=dict())
    rng = np.random.default_rng(99)
    sizes = [(480, 640), (301, 999), (776, 554)]
    items = [R.item("nv12", H, W, R.random_planes("nv12", H, W, rng)) for H, W in sizes]
    rgb = [R.to_rgb(it, "nv12") for it in items]
    before = dict(_cabi.CALLS)
    got = inf(items, input_format="nv12", device=DEV, dtype=dtype, batch_size=2, return_vis=True, pred_score_thr=0.0)
    assert _cabi.CALLS["frames_to_rgb"] - before["frames_to_rgb"] == 2
    assert _cabi.CALLS["preprocess_batch"] - before["preprocess_batch"] == 2
    _equal_results(got, inf(rgb, device=DEV, dtype=dtype, batch_size=2, return_vis=True, pred_score_thr=0.0))
    # (the planes of a GPU-resident frame are views of one surface: the odd-sized frame's tuple is uploaded as one)
    on_gpu = [_resident_planes(it) if isinstance(it, tuple) else torch.from_numpy(it).to(DEV) for it in items]
    _equal_results(inf(on_gpu, input_format="nv12", device=DEV, dtype=dtype, batch_size=2, return_vis=True,
                       pred_score_thr=0.0), got)
    assert len(got["predictions"]) == 3 and sum(len(p["labels"]) for p in got["predictions"]) > 0


def _resident_planes(planes):
    """a tuple of host planes (y, uv) as views of one GPU buffer"""
    y, uv = planes
    flat = torch.from_numpy(np.concatenate((y.reshape(-1), uv.reshape(-1)))).to(DEV)
    return flat[:y.size].view(y.shape), flat[y.size:].view(uv.shape)
