"""GPU: the JPEG encoder -- codetr_jpeg_encode_u8 (csrc/jpeg.hip) and hip_ops.encode_jpeg byte for byte against the numpy
restatement of the header's rule (tests/jpeg_ref.py, pinned to Pillow in test_jpeg_cpu.py; integer arithmetic, no
tolerance), and `Inferencer(vis_format="jpeg")` end to end with a stub model: the files are the restatement's encoding
of the arrays the same call returns, and without `return_vis` the RGB buffer never leaves the GPU."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases as C
import jpeg_ref as J
from test_inferencer_batch_gpu import DEV

pytestmark = pytest.mark.gpu
GUARD = 64


def _buffer(images, seed=5):
    """the images in one flat buffer at odd byte offsets with random bytes between -> (numpy buffer, rows)"""
    rng = np.random.default_rng(seed)
    rows, offset = [], 1
    for i, im in enumerate(images):
        rows.append((offset, im.shape[0], im.shape[1]))
        offset += im.size + (3, 5, 2)[i % 3]
    buf = rng.integers(0, 256, offset + GUARD, dtype=np.uint8)
    for (o, H, W), im in zip(rows, images):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, rows


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("quality,sub", C.GROUPS)
def test_files_equal_the_restatement(quality, sub):
    """every shape and content of the group in one call: 1x1 .. 33x31, the ten-row image (RST wrap), the 4112-wide
    image (ten passes per workgroup), at odd offsets in one buffer"""
    from codetr import _cabi, hip_ops

    cases = C.group(quality, sub)
    expect, _ = C.expected(quality, sub)
    buf, rows = _buffer([im for _, im in cases])
    dev = torch.from_numpy(buf).to(DEV)
    before = _cabi.CALLS["jpeg_encode"]
    got = hip_ops.encode_jpeg(dev, rows, quality, sub)
    assert _cabi.CALLS["jpeg_encode"] - before >= 1 and len(got) == len(cases)
    assert np.array_equal(dev.cpu().numpy(), buf)          # the source is only read
    for (name, _), a, b in zip(cases, got, expect):
        assert isinstance(a, bytes) and a == b, (name, len(a), len(b))


def test_three_images_of_different_sizes_in_one_launch():
    from codetr import _jpeg

    images = [C.content("noise", 53, 37, 1), C.content("gradient", 130, 9, 2), C.content("checker", 48, 64, 3)]
    buf, rows = _buffer(images, 6)
    assert all(o % 2 for o, _, _ in rows[:2])
    dev = torch.from_numpy(buf).to(DEV)
    stride = 20000
    out = torch.full((3 * stride + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty((_jpeg.workspace_bytes(rows, 0, stride),), dtype=torch.uint8, device=DEV)
    _jpeg.encode(dev, rows, 75, 0, out, stride, lengths, ws)
    host, n = out.cpu().numpy(), lengths.cpu().numpy()
    for k, im in enumerate(images):
        ref = J.encode(im, 75, "420")
        assert host[k * stride:k * stride + n[k]].tobytes() == ref[629:-2], k
        assert (host[k * stride + n[k]:(k + 1) * stride] == 0xA5).all(), k       # nothing behind the scan
    assert (host[3 * stride:] == 0xA5).all()


def test_thirty_three_images_take_two_launch_groups():
    from codetr import _cabi, hip_ops

    images = [C.content("noise", 16, 16, 100 + i) for i in range(33)]
    buf, rows = _buffer(images, 7)
    before, copies = _cabi.CALLS["jpeg_encode"], hip_ops.JPEG_DOWNLOADS["copies"]
    got = hip_ops.encode_jpeg(torch.from_numpy(buf).to(DEV), rows, 90, "420")
    assert _cabi.CALLS["jpeg_encode"] == before + 2 and hip_ops.JPEG_DOWNLOADS["copies"] == copies + 2
    assert got == [J.encode(im, 90, "420") for im in images]


def test_capacity():
    """a slot too small: length -1, the slot, the guard and the neighbours' bytes untouched, the others correct"""
    from codetr import _cabi, _jpeg, hip_ops

    images = [C.content("gradient", 40, 40, 1), C.content("noise", 40, 40, 2), C.content("zeros", 40, 40, 3)]
    refs = [J.encode(im, 100, "444")[629:-2] for im in images]
    buf, rows = _buffer(images, 8)
    dev = torch.from_numpy(buf).to(DEV)
    stride = len(refs[1]) - 1                       # one byte short for the noise image
    assert len(refs[0]) < stride and len(refs[2]) < stride
    for s, fits in ((stride, (True, False, True)), (stride + 1, (True, True, True)), (len(refs[2]) - 1, (False,) * 3)):
        out = torch.full((3 * s + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        lengths = torch.full((3,), -7, dtype=torch.int32, device=DEV)
        ws = torch.empty((_jpeg.workspace_bytes(rows, 1, s),), dtype=torch.uint8, device=DEV)
        _jpeg.encode(dev, rows, 100, 1, out, s, lengths, ws)
        host, n = out.cpu().numpy(), lengths.cpu().numpy()
        assert (host[3 * s:] == 0xA5).all()
        for k in range(3):
            slot = host[k * s:(k + 1) * s]
            if fits[k]:
                assert n[k] == len(refs[k]) and slot[:n[k]].tobytes() == refs[k] and (slot[n[k]:] == 0xA5).all(), (s, k)
            else:
                assert n[k] == -1 and (slot == 0xA5).all(), (s, k)
    # hip_ops: the image that does not fit the first attempt is encoded once more, at the proven bound
    before, copies = _cabi.CALLS["jpeg_encode"], hip_ops.JPEG_DOWNLOADS["copies"]
    got = hip_ops.encode_jpeg(dev, rows, 100, "444", out_stride=stride)
    assert _cabi.CALLS["jpeg_encode"] == before + 2 and hip_ops.JPEG_DOWNLOADS["copies"] == copies + 2
    assert [g[629:-2] for g in got] == refs and all(g == J.encode(im, 100, "444") for g, im in zip(got, images))
    # the default reservation (an eighth of the raw size + 4 KB) is too small for noise at quality 100 at this size
    big = C.content("noise", 160, 120, 4)
    assert len(J.encode(big, 100, "444")) > hip_ops.jpeg_out_stride([(0, 120, 160)], "444")
    before = _cabi.CALLS["jpeg_encode"]
    assert hip_ops.encode_jpeg(torch.from_numpy(big).to(DEV).view(-1), [(0, 120, 160)], 100, "444") == [J.encode(big, 100, "444")]
    assert _cabi.CALLS["jpeg_encode"] == before + 2


def test_a_rejected_call_writes_nothing():
    from codetr import _jpeg

    dev = torch.zeros((16 * 16 * 3,), dtype=torch.uint8, device=DEV)
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty((_jpeg.workspace_bytes([(0, 16, 16)], 0, 4096),), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="codetr_jpeg_encode_u8"):
        _jpeg.encode(dev, [(0, 16, 16)], 101, 0, out, 4096, lengths, ws)
    with pytest.raises(RuntimeError, match="codetr_jpeg_encode_u8"):
        _jpeg.encode(dev, [(1, 16, 16)], 90, 0, out, 4096, lengths, ws)           # the image ends outside the buffer
    with pytest.raises(RuntimeError, match="codetr_jpeg_encode_u8"):
        _jpeg.encode(dev, [(0, 16, 16)], 90, 0, out, 4096, lengths, ws[:-1])       # a workspace one byte short
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all() and int(lengths.cpu()[0]) == -7


# ---- 2. the Inferencer --------------------------------------------------------------------------------------------------------
SIZES = [(120, 160), (37, 53), (96, 200), (64, 48), (150, 90)]
PATHS = {
    "plain": dict(),
    "soft": dict(nms_type="config"),
    "tta": dict(tta=dict(scales=[(320, 200), (400, 256)], flip=True, max_per_img=50)),
    "sliced": dict(slicing=dict(tile=(100, 80), tile_batch=8, max_per_img=100)),
    "tracked": dict(tracker={}),
}


def _inferencer(**kw):
    from codetr.inferencer import Inferencer
    from test_inferencer_batch_gpu import SWIN
    from test_tta_gpu import _stub

    inf = Inferencer(_stub([]), SWIN, dataset_meta=None, score_threshold=0.3, visualizer=dict(), **kw)
    inf.scale = (400, 256)      # (small inputs, as in test_frames_gpu.py)
    inf.pad_size = None
    return inf


def _smooth(shape, rng):
    """a ramp with +-4 of noise: compresses like a photograph, so the first reservation of encode_jpeg holds"""
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    ramp = (xx * int(rng.integers(1, 4)) + yy * int(rng.integers(1, 4))) % 256
    ramp = ramp[..., None] + np.arange(0, 40 * shape[2], 40) if len(shape) == 3 else ramp
    return np.clip(ramp % 256 + rng.integers(-4, 5, shape), 0, 255).astype(np.uint8)


def _items(fmt, seed):
    import frames_ref as R

    rng = np.random.default_rng(seed)
    if fmt in ("rgb", "bgr"):
        images = [_smooth((H, W, 3), rng) for H, W in SIZES]
        return images if fmt == "rgb" else [im[..., ::-1] for im in images]
    return [R.item(fmt, H, W, [_smooth(shape, rng) for shape in R.plane_shapes(fmt, H, W)]) for H, W in SIZES]


@pytest.mark.parametrize("path", list(PATHS))
def test_inferencer_writes_the_restatements_jpeg(path, tmp_path, monkeypatch):
    from codetr import _cabi, inferencer

    fmt = dict(plain="rgb", soft="nv12", tta="bgr", sliced="i420", tracked="rgb")[path]
    settings = dict(type="jpeg", quality=85, subsampling="444") if path == "soft" else "jpeg"
    q, sub = (85, "444") if path == "soft" else (90, "420")
    items = _items(fmt, 90)
    call = dict(input_format=fmt, batch_size=3, pred_score_thr=0.4, device=DEV, dtype=torch.float16)
    inf = _inferencer(vis_format=settings, **PATHS[path])
    out = inf(items, return_vis=True, out_dir=str(tmp_path / "a"), **call)
    arrays = out["visualization"]
    assert len(arrays) == len(items) and "visualization_jpeg" not in out
    assert sorted(os.listdir(tmp_path / "a" / "vis")) == ["%08d.jpg" % i for i in range(len(items))]
    files = [open(tmp_path / "a" / "vis" / ("%08d.jpg" % i), "rb").read() for i in range(len(items))]
    for i, (arr, data) in enumerate(zip(arrays, files)):
        assert arr.shape == SIZES[i] + (3,) and data == J.encode(arr, q, sub), i
    # without return_vis: the same files, and the chunk's RGB buffer is never downloaded
    sizes = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (sizes.append((t.dtype, t.numel())), real(t, *a, **k))[1])
    inf = _inferencer(vis_format=settings, **PATHS[path])
    rgb_before, calls = inferencer.VIS_DOWNLOADS["rgb"], _cabi.CALLS["jpeg_encode"]
    out = inf(items, out_dir=str(tmp_path / "b"), **call)
    monkeypatch.undo()
    assert out["visualization"] == [] and inferencer.VIS_DOWNLOADS["rgb"] == rgb_before
    # what encode_jpeg had to fetch, from its stated rule: per chunk of 3 one buffer of 16 bytes of lengths + a slot of
    # jpeg_out_stride per image, and, where a scan does not fit its slot, one more for those images at the proven bound
    from codetr import _jpeg, hip_ops
    expect_calls, expect_sizes = 0, []
    for i in (0, 3):
        hw, scans = SIZES[i:i + 3], [len(f) - 631 for f in files[i:i + 3]]
        stride = hip_ops.jpeg_out_stride([(0, H, W) for H, W in hw], sub)
        missed = [k for k, n in enumerate(scans) if n > stride]
        expect_calls += 1 + bool(missed)
        expect_sizes.append(16 + len(hw) * stride)
        if missed:
            bound = max(_jpeg.scan_bound(hw[k][0], hw[k][1], _jpeg.SUBSAMPLINGS[sub]) for k in missed)
            expect_sizes.append(16 + len(missed) * ((bound + 15) // 16 * 16))
    assert _cabi.CALLS["jpeg_encode"] == calls + expect_calls
    # every other byte buffer that came back (the packed detections) is smaller than the images of either chunk, which a
    # download of a chunk's RGB buffer would at least hold: no RGB left the GPU
    u8 = [n for dt, n in sizes if dt == torch.uint8]
    assert sorted(n for n in u8 if n in expect_sizes) == sorted(expect_sizes), (sizes, expect_sizes)
    smaller_chunk = min(sum(H * W * 3 for H, W in SIZES[i:i + 3]) for i in (0, 3))
    assert all(n < smaller_chunk for n in u8 if n not in expect_sizes), (sizes, expect_sizes)
    assert [open(tmp_path / "b" / "vis" / ("%08d.jpg" % i), "rb").read() for i in range(len(items))] == files
    # return_vis="jpeg": the files as bytes objects, nothing on disk
    inf = _inferencer(vis_format=settings, **PATHS[path])
    out = inf(items, return_vis="jpeg", **call)
    assert out["visualization_jpeg"] == files and out["visualization"] == []
    assert inf.num_visualized_imgs == len(items)


def test_undrawn_frames_and_the_png_default(tmp_path):
    """draw_pred=False encodes the converted frames as they are; vis_format=None writes the PNG files it always wrote"""
    import frames_ref as R
    from codetr import _cabi, inferencer
    from test_draw_cpu import read_png

    items = _items("nv12", 91)
    rgb = [R.to_rgb(it, "nv12") for it in items]
    call = dict(input_format="nv12", batch_size=5, device=DEV, dtype=torch.float16)
    inf = _inferencer(vis_format="jpeg")
    before = _cabi.CALLS["draw_detections"]
    out = inf(items, return_vis="jpeg", draw_pred=False, **call)
    assert _cabi.CALLS["draw_detections"] == before
    assert out["visualization_jpeg"] == [J.encode(im, 90, "420") for im in rgb]
    # the default: PNG, byte for byte what write_png makes of the returned arrays, and no encoder launch
    for fmt in (None, "png"):
        inf = _inferencer(vis_format=fmt)
        calls = _cabi.CALLS["jpeg_encode"]
        d = tmp_path / str(fmt)
        out = inf(items, return_vis=True, out_dir=str(d), **call)
        assert _cabi.CALLS["jpeg_encode"] == calls
        assert sorted(os.listdir(d / "vis")) == ["%08d.png" % i for i in range(len(items))]
        for i, arr in enumerate(out["visualization"]):
            path = d / "vis" / ("%08d.png" % i)
            assert np.array_equal(read_png(str(path)), arr)
            inferencer.write_png(str(tmp_path / "again.png"), arr)
            assert open(path, "rb").read() == open(tmp_path / "again.png", "rb").read()
    with pytest.raises(ValueError, match="vis_format"):
        inf(items, return_vis="jpeg", **call)
