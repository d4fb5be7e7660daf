"""GPU: the JPEG decoder -- codetr_jpegdec_decode_u8 (csrc/jpeg_dec.hip), hip_ops.decode_jpeg and
`Inferencer(...)(files, input_format="jpeg")` byte for byte against the numpy restatement of the header's rule
(tests/jpeg_dec_ref.py, pinned to Pillow in test_jpeg_dec_cpu.py; integer arithmetic, no tolerance).  The files are the
committed ones of tests/golden/jpeg_dec; the corrupt scans are those test_jpeg_dec_cpu.py first runs through the host
memory check."""
import numpy as np
import pytest
import torch

import jpeg_dec_cases as C
import jpeg_dec_ref as D
from test_inferencer_batch_gpu import DEV

pytestmark = pytest.mark.gpu
GUARD = 48


def _launch(files, seed=3):
    """the files' scans at odd offsets in one buffer with random bytes between, one call of the entry point into slots
    with guard bytes around them -> (images, status words, launch count)"""
    from codetr import _cabi, _jpeg_dec

    rng = np.random.default_rng(seed)
    parsed = []
    for f in files:
        rc, info, tables = _jpeg_dec.parse(np.frombuffer(f, np.uint8))
        assert rc == 0
        parsed.append((info, tables))
    rows, at, dst = [], 1, GUARD + 1
    for f, (info, _) in zip(files, parsed):
        rows.append((at, int(info[5]), int(info[0]), int(info[1]), dst))
        at += int(info[5]) + (3, 6, 1)[len(rows) % 3]
        dst += int(info[0]) * int(info[1]) * 3 + GUARD
    at += (-at) % 16
    src = rng.integers(0, 256, at + len(files) * _jpeg_dec.TABLE_BYTES, dtype=np.uint8)
    for f, (info, tables), r, k in zip(files, parsed, rows, range(len(files))):
        src[r[0]:r[0] + r[1]] = np.frombuffer(f, np.uint8)[int(info[4]):int(info[4]) + r[1]]
        src[at + k * _jpeg_dec.TABLE_BYTES:at + (k + 1) * _jpeg_dec.TABLE_BYTES] = tables
    dev = torch.from_numpy(src).to(DEV)
    out = torch.full((dst,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((len(files),), -7, dtype=torch.int32, device=DEV)
    infos = np.stack([p[0] for p in parsed])
    ws = torch.empty((_jpeg_dec.workspace_bytes(rows, infos),), dtype=torch.uint8, device=DEV)
    before = _cabi.CALLS["jpeg_decode"]
    _jpeg_dec.decode(dev, rows, infos, dev[at:], out, status, ws)
    host = out.cpu().numpy()
    assert np.array_equal(dev.cpu().numpy(), src)          # the scans and tables are only read
    images, edge = [], 0
    for r in rows:
        assert (host[edge:r[4]] == 0xA5).all(), "guard bytes in front of an image were written"
        edge = r[4] + r[2] * r[3] * 3
        images.append(host[r[4]:edge].reshape(r[2], r[3], 3))
    assert (host[edge:] == 0xA5).all(), "guard bytes behind the last image were written"
    return images, status.cpu().numpy().tolist(), _cabi.CALLS["jpeg_decode"] - before


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", C.GROUPS)
def test_files_equal_the_restatement(sub):
    """every supported file of one subsampling in one call: 1x1 .. 37x53, replication (dw <= 2) and the fancy rule, every
    table and restart option; at 4:2:0 also the two 320x240 files (many chunks, more than one run)"""
    names = C.group(sub)
    assert len(names) >= 8
    images, status, calls = _launch([C.data(n) for n in names])
    assert calls == 1 and status == [0] * len(names)
    for n, got in zip(names, images):
        assert np.array_equal(got, C.expected(n)[0]), n


def test_the_noise_file_takes_many_rounds_and_more_than_one_run():
    from codetr import _jpeg_dec, hip_ops

    info = D.parse(C.data(C.NOISE))
    assert info["scan_bytes"] > 4 * _jpeg_dec.CHUNK_BYTES * _jpeg_dec.RUN_CHUNKS and info["dri"] == 0
    buf, staged = hip_ops.decode_jpeg([C.data(C.NOISE)])
    assert staged == [(0, 240, 320)]
    assert np.array_equal(buf.cpu().numpy()[:240 * 320 * 3].reshape(240, 320, 3), C.expected(C.NOISE)[0])


def test_thirty_three_files_take_two_launch_groups(tmp_path):
    from codetr import _cabi, hip_ops

    names = [n for n in C.SUPPORTED if "320x240" not in n][:33]
    assert len(names) == 33
    files = [C.data(n) for n in names]
    # every kind of argument decode_jpeg takes
    path = tmp_path / "a.jpg"
    path.write_bytes(files[0])
    files[0], files[1], files[2] = str(path), bytearray(files[1]), memoryview(files[2])
    files[3], files[4], files[5] = np.frombuffer(files[3], np.uint8), torch.frombuffer(bytearray(files[4]), dtype=torch.uint8), path
    before = _cabi.CALLS["jpeg_decode"]
    buf, staged = hip_ops.decode_jpeg(files)
    assert _cabi.CALLS["jpeg_decode"] == before + 2
    host = buf.cpu().numpy()
    files[5] = C.data(names[0])
    for k, (n, (o, H, W)) in enumerate(zip(names, staged)):
        exp = C.expected(names[0] if k == 5 else n)[0]
        assert o % 16 == 0 and (H, W) == exp.shape[:2]
        assert np.array_equal(host[o:o + H * W * 3].reshape(H, W, 3), exp), n


def test_the_encoders_ten_row_file():
    """the project's own encoder: one restart interval per MCU row, ten rows, so RST7 is followed by RST0"""
    f = C.encoder_file()
    assert f.count(b"\xff\xd0") >= 2 and b"\xff\xd7" in f
    exp, status = D.decode(f)
    assert status == 0
    images, got_status, _ = _launch([f], 4)
    assert got_status == [0] and np.array_equal(images[0], exp)


def test_corrupt_scans_get_the_predicted_status():
    """five corrupt scans between good files: each gets the status the restatement predicts, the good images are right,
    every write stays inside its image (the guards of _launch)"""
    bad = C.corrupt()
    good = ["444_8x8_q90_opt", "420_17x9_q100", "grey_16x16_q100"]
    order = [good[0]] + list(bad)[:2] + [good[1]] + list(bad)[2:] + [good[2]]
    predicted = [C.expected(n)[1] for n in order]
    assert all(predicted[order.index(n)] != 0 for n in bad) and len(bad) == 5
    images, status, _ = _launch([bad[n] if n in bad else C.data(n) for n in order], 5)
    assert status == predicted
    for n, got in zip(order, images):
        if n not in bad:
            assert np.array_equal(got, C.expected(n)[0]), n
    with pytest.raises(ValueError, match="image 1.*index"):
        from codetr import hip_ops
        hip_ops.decode_jpeg([C.data(good[0]), bad["corrupt_flip_420"]])


def test_a_rejected_call_writes_nothing():
    from codetr import _jpeg_dec

    f = np.frombuffer(C.data("420_16x16_q90_rb3"), np.uint8)
    rc, info, tables = _jpeg_dec.parse(f)
    scan = f[int(info[4]):int(info[4]) + int(info[5])]
    src = torch.from_numpy(np.concatenate([scan, np.zeros((-scan.size) % 16, np.uint8), tables])).to(DEV)
    at = src.numel() - _jpeg_dec.TABLE_BYTES
    out = torch.full((16 * 16 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    row = (0, scan.size, 16, 16, 0)
    ws = torch.empty((_jpeg_dec.workspace_bytes([row], info),), dtype=torch.uint8, device=DEV)

    class Null:
        device = src.device

        def data_ptr(self):
            return 0

        def numel(self):
            return src.numel()

    calls = [lambda: _jpeg_dec.decode(Null(), [row], info, src[at:], out, status, ws),               # a null pointer
             lambda: _jpeg_dec.decode(src, [(at, scan.size + src.numel(), 16, 16, 0)], info, src[at:], out, status, ws),
             lambda: _jpeg_dec.decode(src, [(0, scan.size, 16, 16, 1)], info, src[at:], out, status, ws),  # ends outside
             lambda: _jpeg_dec.decode(src, [row], info, src[at:], out, status, ws[:-1])]             # a workspace one byte short
    for call in calls:
        with pytest.raises(RuntimeError, match="codetr_jpegdec_decode_u8"):
            call()
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all() and int(status.cpu()[0]) == -7
    _jpeg_dec.decode(src, [row], info, src[at:], out, status, ws)
    assert int(status.cpu()[0]) == 0 and np.array_equal(out.cpu().numpy().reshape(16, 16, 3), C.expected("420_16x16_q90_rb3")[0])


# ---- 2. the Inferencer --------------------------------------------------------------------------------------------------------
FILES = ["420_37x53_q30_opt_rb3", "444_33x31_q90_rb3", "refuse_progressive", "grey_37x53_q100_rr1", "422_37x53_q90"]


def _inferencer(**kw):
    from test_jpeg_gpu import _inferencer as make

    return make(**kw)


def _progressive_rgb():
    """the progressive file as the host fallback decodes it: Pillow where it imports (then the test holds the fallback
    to it), else the file is left out of the comparison"""
    try:
        import io

        from PIL import Image
    except ImportError:
        return None
    return np.asarray(Image.open(io.BytesIO(C.data("refuse_progressive"))).convert("RGB"))


def test_inferencer_takes_jpeg_files():
    from codetr import _cabi, hip_ops

    prog = _progressive_rgb()
    names = FILES if prog is not None else [n for n in FILES if n != "refuse_progressive"]
    files = [C.data(n) for n in names]
    arrays = [prog if n == "refuse_progressive" else np.array(C.expected(n)[0]) for n in names]
    call = dict(batch_size=3, pred_score_thr=0.4, device=DEV, dtype=torch.float16, return_vis=True)
    calls, falls = _cabi.CALLS["jpeg_decode"], hip_ops.JPEG_DECODE_STATS["host_fallbacks"]
    out = _inferencer()(files, input_format="jpeg", **call)
    assert _cabi.CALLS["jpeg_decode"] == calls + 2                      # one launch group per chunk of 3
    assert hip_ops.JPEG_DECODE_STATS["host_fallbacks"] == falls + (prog is not None)
    ref = _inferencer()(arrays, input_format="rgb", **call)
    assert out["predictions"] == ref["predictions"] and len(out["predictions"]) == len(names)
    assert any(len(p["labels"]) for p in out["predictions"])
    for a, b in zip(out["visualization"], ref["visualization"]):
        assert np.array_equal(a, b)
    # a corrupt file: a ValueError that names the image, raised behind the chunk's download
    bad = [files[0], C.corrupt()["corrupt_cut_422"], files[1]]
    with pytest.raises(ValueError, match="image 1.*exhausted"):
        _inferencer()(bad, input_format="jpeg", **call)
    # an unsupported file without the host decoder: the reason
    if prog is None:
        with pytest.raises(ValueError, match="progressive"):
            _inferencer()([C.data("refuse_progressive")], input_format="jpeg", **call)
    with pytest.raises(ValueError, match="input_format must be one of"):
        _inferencer()(files, input_format="jpg", **call)


@pytest.mark.parametrize("path", ["tta", "sliced", "tracked"])
def test_inferencer_paths_take_jpeg_files(path):
    """the TTA and slicing tails ride in the same staging copy as the scans; the predictions are those of the arrays"""
    from test_jpeg_gpu import PATHS

    names = [n for n in FILES if n != "refuse_progressive"]
    call = dict(batch_size=3, device=DEV, dtype=torch.float16)
    out = _inferencer(**PATHS[path])([C.data(n) for n in names], input_format="jpeg", **call)
    ref = _inferencer(**PATHS[path])([np.array(C.expected(n)[0]) for n in names], input_format="rgb", **call)
    assert out["predictions"] == ref["predictions"] and len(out["predictions"]) == len(names)


def test_preprocess_batch_takes_jpeg_files():
    inf = _inferencer()
    names = [n for n in FILES if n != "refuse_progressive"]
    x, m, metas = inf.preprocess_batch([C.data(n) for n in names], device=DEV, dtype=torch.float16, input_format="jpeg")
    inf.check_jpeg_status()
    xr, mr, metas_r = inf.preprocess_batch([np.array(C.expected(n)[0]) for n in names], device=DEV, dtype=torch.float16)
    assert torch.equal(x, xr) and torch.equal(m, mr) and metas == metas_r
    inf.preprocess_batch([C.corrupt()["corrupt_cut_422"]], device=DEV, dtype=torch.float16, input_format="jpeg")
    with pytest.raises(ValueError, match="image 0.*exhausted"):
        inf.check_jpeg_status()
