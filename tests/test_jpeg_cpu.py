"""CPU: the JPEG file format of include/codetr_jpeg.h -- the structure of the files the numpy restatement
(tests/jpeg_ref.py) writes, the restatement's own decoder, the coverage of the GPU test's case list, the restatement
pinned to Pillow (tables byte for byte; quality and size against Pillow's own encoder), the host-only entry points of
the built library, and the `vis_format` settings of the Inferencer."""
import ctypes
import io
import os

import numpy as np
import pytest

import jpeg_cases as C
import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scan_markers(data):
    """the scan of a file -> the RST numbers in it, after checking that FF is followed by 00 or RSTm only"""
    _, p = J.segments(data)
    scan, rst, i = data[p:-2], [], 0
    while i < len(scan):
        if scan[i] == 0xFF:
            assert i + 1 < len(scan) and (scan[i + 1] == 0 or 0xD0 <= scan[i + 1] <= 0xD7), i
            if scan[i + 1]:
                rst.append(scan[i + 1] - 0xD0)
            i += 2
        else:
            i += 1
    return rst


# ---- 1. structure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (40, 147), (129, 33)])
def test_file_structure(W, H, sub):
    data = J.encode(C.content("noise", W, H), 90, sub)
    segs, p = J.segments(data)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert [len(b) + 2 for _, b in segs] == [16, 67, 67, 17, 31, 181, 31, 181, 4, 12] and p == 629
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    assert segs[0][1] == b"JFIF\0\1\1\0\0\1\0\1\0\0"
    sof = segs[3][1]
    assert sof[0] == 8 and (int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big")) == (H, W)
    assert sof[5:] == bytes([3, 1, 0x22 if sub == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [b[0] for _, b in segs[4:8]] == [0x00, 0x10, 0x01, 0x11] and [segs[1][1][0], segs[2][1][0]] == [0, 1]
    px = 16 if sub == "420" else 8
    assert int.from_bytes(segs[8][1], "big") == -(-W // px)                  # DRI = MCUs per row
    assert segs[9][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    rows = -(-H // px)
    assert _scan_markers(data) == [r % 8 for r in range(rows - 1)]           # cycles 0..7, wraps, none after the last


def test_the_typed_dct_matrix_is_the_headers():
    text = open(os.path.join(ROOT, "include", "codetr_jpeg.h")).read()
    for k in range(8):
        line = next(ln for ln in text.splitlines() if ln.strip().startswith(f"*     k = {k}:"))
        assert [int(v) for v in line.split(":")[1].split()] == J.DCT[k].tolist()


def test_reciprocal_division_is_exact():
    """the kernel divides by a quantiser t with (a * (2^20 / t + 1)) >> 20: exact for every a it can meet"""
    a = np.arange(4096, dtype=np.int64)
    for t in range(1, 256):
        assert np.array_equal((a * ((1 << 20) // t + 1)) >> 20, a // t)


# ---- 2. the restatement's decoder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", ["420", "444"])
def test_round_trip_psnr_rises_with_quality(sub):
    img = _gradient_noise(61, 83)
    got = []
    for q in (5, 25, 50, 75, 90, 100):
        out = J.decode(J.encode(img, q, sub))
        assert out.shape == img.shape and out.dtype == np.uint8
        got.append(J.psnr(out, img))
    assert all(b > a for a, b in zip(got, got[1:])) and got[0] > 20 and got[-1] > 35, got


# ---- 3. the GPU test's case list reaches every branch ----------------------------------------------------------------------
def test_case_list_coverage():
    total = J.new_stats()
    for q, s in C.GROUPS:
        files, stats = C.expected(q, s)
        assert len(files) == len(C.group(q, s)) > 0
        for k, v in stats.items():
            total[k] = total[k] | v if isinstance(v, set) else total[k] + v
        for data in files:   # no FF in a scan is followed by anything but 00 or RSTm
            _scan_markers(data)
    assert total["zrl"] > 0 and total["no_eob"] > 0 and total["stuffed"] > 0
    assert 11 in total["dc_categories"] and total["negative_dc"] > 0 and total["zero_dc"] > 0
    assert {q for q, _ in C.GROUPS} >= {1, 10, 50, 90, 100} and {s for _, s in C.GROUPS} == {"420", "444"}
    shapes = set(C.SHAPES)
    assert {(1, 1), (8, 8), (16, 16), (17, 9), (33, 31), (40, 147), (40, 75)} <= shapes
    assert any(-(-H // 16) >= 9 for W, H in shapes) and any(-(-H // 8) >= 9 for W, H in shapes)      # the RST wrap
    assert any(W % 16 and H % 16 for W, H in shapes)                                                # partial MCUs, both axes
    from codetr import _jpeg
    assert any(W > _jpeg.PASS_PIXELS and W % _jpeg.PASS_PIXELS for W, H in shapes)   # more than one pass, a short last one
    # every group has the 40-wide ten-row image of its subsampling
    for q, s in C.GROUPS:
        assert any(name.endswith("40x147" if s == "420" else "40x75") for name, _ in C.group(q, s))


# ---- 4. pinned to Pillow -----------------------------------------------------------------------------------------------------
def _gradient_noise(H, W):
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[:H, :W]
    img = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (W + H - 2)], -1)
    return np.clip(img + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)


def _box_scene(H, W):
    """flat regions, outlines three pixels wide and small dark patches: what the drawing kernel produces"""
    rng = np.random.default_rng(8)
    img = np.empty((H, W, 3), np.uint8)
    img[:] = (90, 120, 150)
    img[H // 2:] = (60, 140, 70)
    for _ in range(12):
        x0, y0 = int(rng.integers(0, W - 40)), int(rng.integers(0, H - 40))
        w, h = int(rng.integers(20, W // 2)), int(rng.integers(20, H // 2))
        x1, y1 = min(W - 1, x0 + w), min(H - 1, y0 + h)
        c = rng.integers(0, 256, 3)
        for t in range(3):
            img[y0 + t, x0:x1 + 1] = c
            img[y1 - t, x0:x1 + 1] = c
            img[y0:y1 + 1, x0 + t] = c
            img[y0:y1 + 1, x1 - t] = c
        img[y0 + 3:y0 + 12, x0 + 3:min(x1, x0 + 60)] //= 4
    return img


def _pillow(img, q, sub):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling={"420": 2, "444": 0}[sub], optimize=False)
    return b.getvalue()


def _pillow_decode(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _tables(data):
    """{('q' | 'h', id): payload} of every table of a file, whether its segments hold one table or several"""
    out, p = {}, 2
    while True:
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        body, i = data[p + 4:p + 2 + n], 0
        while m in (0xC4, 0xDB) and i < len(body):
            size = 65 if m == 0xDB else 17 + sum(body[i + 1:i + 17])
            out[("q" if m == 0xDB else "h", body[i])] = body[i + 1:i + size]
            i += size
        p += 2 + n
        if m == 0xDA:
            return out


def test_pillow_opens_every_file():
    pytest.importorskip("PIL")
    for q, s in C.GROUPS:
        for (name, img), data in zip(C.group(q, s), C.expected(q, s)[0]):
            out = _pillow_decode(data)
            assert out.shape == img.shape, name
            if name.startswith(("zeros", "ones")):
                assert np.abs(out.astype(int) - img).max() <= 2, name


@pytest.mark.parametrize("q", [1, 10, 37, 50, 75, 90, 100])
def test_tables_are_pillows(q):
    pytest.importorskip("PIL")
    img = _gradient_noise(24, 24)
    ours, theirs = _tables(J.encode(img, q, "420")), _tables(_pillow(img, q, "420"))
    assert sorted(ours) == sorted(theirs) == [("h", 0x00), ("h", 0x01), ("h", 0x10), ("h", 0x11), ("q", 0), ("q", 1)]
    for key in ours:
        assert ours[key] == theirs[key], key


# Measured with Pillow 12 / libjpeg-turbo on the two images below, (PSNR after Pillow's decode in dB, file bytes), the
# restatement's file first, Pillow's own second:
PILLOW_PAIRS = {
    ("gradient", 50, "420"): ((35.95, 2586), (35.98, 2524)),     # -0.03 dB, +2.5 %
    ("gradient", 50, "444"): ((35.88, 3631), (35.90, 3519)),     # -0.02 dB, +3.2 %
    ("gradient", 90, "420"): ((36.65, 8881), (36.73, 8534)),     # -0.08 dB, +4.1 %
    ("gradient", 90, "444"): ((37.01, 12590), (37.07, 12156)),   # -0.06 dB, +3.6 %
    ("boxes", 50, "420"): ((25.71, 5207), (25.71, 5158)),        #  0.00 dB, +1.0 %
    ("boxes", 50, "444"): ((30.50, 7491), (30.50, 7384)),        #  0.00 dB, +1.4 %
    ("boxes", 90, "420"): ((27.66, 10117), (27.63, 10041)),      # +0.03 dB, +0.8 %
    ("boxes", 90, "444"): ((39.29, 15373), (39.32, 15168)),      # -0.03 dB, +1.4 %
}
PSNR_GAP_DB = max(b[0] - a[0] for a, b in PILLOW_PAIRS.values())     # 0.08 dB
SIZE_GAP = max(a[1] / b[1] - 1 for a, b in PILLOW_PAIRS.values())    # 4.1 %
PSNR_SLACK_DB = 0.15   # see test_quality_and_size_against_pillow
SIZE_SLACK = 0.02


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("scene", ["gradient", "boxes"])
def test_quality_and_size_against_pillow(scene, q, sub):
    """The restatement against Pillow's encoder at the same quality and subsampling, both decoded by Pillow.  The gap has
    known sources -- a restart marker and up to seven pad bits per MCU row plus the DRI segment cost bytes (Pillow writes
    no restart markers); the integer DCT rounds twice where libjpeg-turbo's rounds after descaling; the 2x2 chroma
    mean here rounds (+2) where libjpeg alternates its bias; -- but not a derivable size, so it is measured: the pairs
    above.  Allowed: the largest measured PSNR deficit + 0.15 dB (a tenth of the smallest step between two neighbouring
    qualities of test_round_trip_psnr_rises_with_quality, i.e. far below a visible difference) and the largest measured
    size excess + 2 % of Pillow's size (the header differs by a few dozen bytes between library builds)."""
    pytest.importorskip("PIL")
    img = _gradient_noise(192, 256) if scene == "gradient" else _box_scene(192, 256)
    ours, theirs = J.encode(img, q, sub), _pillow(img, q, sub)
    a, b = J.psnr(_pillow_decode(ours), img), J.psnr(_pillow_decode(theirs), img)
    print(f"{scene} q{q} {sub}: restatement {a:.2f} dB {len(ours)} B, Pillow {b:.2f} dB {len(theirs)} B")
    assert a >= b - PSNR_GAP_DB - PSNR_SLACK_DB
    assert len(ours) <= len(theirs) * (1 + SIZE_GAP + SIZE_SLACK)


# ---- 5. the library's host-only entry points and the binding ----------------------------------------------------------------
def test_header_parses_and_binds():
    from codetr import _cabi, _cheader, _jpeg

    functions, defines = _cheader.parse(open(_jpeg.HEADER_PATH).read())
    assert sorted(functions) == ["codetr_jpeg_abi_version", "codetr_jpeg_encode_u8", "codetr_jpeg_header",
                                 "codetr_jpeg_scan_bound", "codetr_jpeg_workspace_bytes"]
    assert defines["CODETR_JPEG_ABI_VERSION"] == 1 == _jpeg.load().codetr_jpeg_abi_version()
    assert _jpeg.SUBSAMPLINGS == {"420": 0, "444": 1} and _jpeg.HEADER_BYTES == 629 and _jpeg.PASS_PIXELS == 448
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _jpeg.SIGNATURES["codetr_jpeg_encode_u8"] == (i32, [vp, vp, i64, i64, vp, i32, i32, vp, i64, vp, vp, i64])
    assert _jpeg.SIGNATURES["codetr_jpeg_header"] == (i32, [i64, i64, i32, i32, vp, i64])
    assert _jpeg.SIGNATURES["codetr_jpeg_workspace_bytes"] == (i64, [i64, vp, i32, i64])
    # the companion header adds nothing to the main one: its version and its launch entries stay where they were
    assert not set(functions) & set(_cabi.SIGNATURES) and "jpeg_encode" in _cabi.CALLS


@pytest.mark.parametrize("H,W,q,sub", [(1, 1, 1, "420"), (1080, 1920, 90, "420"), (97, 150, 100, "444"),
                                       (16384, 16384, 37, "444"), (9, 17, 50, "420")])
def test_library_header_is_the_restatements(H, W, q, sub):
    from codetr import _jpeg

    assert _jpeg.header(H, W, q, _jpeg.SUBSAMPLINGS[sub]) == J.header(H, W, q, sub)


def test_header_and_query_arguments():
    from codetr import _jpeg

    lib = _jpeg.load()
    buf = (ctypes.c_ubyte * 700)()
    assert lib.codetr_jpeg_header(8, 8, 90, 0, buf, 629) == 629
    for args in [(8, 8, 90, 0, None, 700), (0, 8, 90, 0, buf, 700), (8, 65536, 90, 0, buf, 700), (8, 8, 0, 0, buf, 700),
                 (8, 8, 101, 0, buf, 700), (8, 8, 90, 2, buf, 700), (8, 8, 90, 0, buf, 628)]:
        assert lib.codetr_jpeg_header(*args) == -1, args
    assert _jpeg.scan_bound(1, 1, 0) == 6 * 416 and _jpeg.scan_bound(1, 1, 1) == 3 * 416
    assert _jpeg.scan_bound(1080, 1920, 0) == 68 * 120 * 6 * 416 + 2 * 67
    assert lib.codetr_jpeg_scan_bound(0, 1, 0) == -1 and lib.codetr_jpeg_scan_bound(1, 16385, 0) == -3
    # the workspace: int32 row lengths rounded up to 16, then per row min(416 * blocks, out_stride) rounded up to 16
    assert _jpeg.workspace_bytes([(0, 1, 1)], 0, 100000) == 16 + 2496
    assert _jpeg.workspace_bytes([(0, 1, 1)], 0, 100) == 16 + 112
    assert _jpeg.workspace_bytes([(0, 147, 40), (5, 9, 17)], 0, 1 << 20) == 48 + 10 * 3 * 2496 + 2 * 2496
    table = (ctypes.c_int64 * 3)(0, 8, 8)
    assert lib.codetr_jpeg_workspace_bytes(0, table, 0, 100) == -1 and lib.codetr_jpeg_workspace_bytes(33, table, 0, 100) == -3
    assert lib.codetr_jpeg_workspace_bytes(1, None, 0, 100) == -1 and lib.codetr_jpeg_workspace_bytes(1, table, 0, 0) == -1


def test_encode_argument_errors_return_before_any_launch():
    """every check runs before the first HIP call, so fake device pointers are never touched -- and this needs no GPU"""
    from codetr import _jpeg

    lib = _jpeg.load()
    one, ws = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    table = (ctypes.c_int64 * 6)(1, 16, 16, 1000, 9, 17)
    need = lib.codetr_jpeg_workspace_bytes(2, table, 0, 4096)

    def call(**kw):
        a = dict(stream=None, buf=one, buf_bytes=2000, N=2, images=table, quality=90, sub=0, out=one, stride=4096, lengths=one,
                 ws=ws, ws_bytes=need)
        a.update(kw)
        return lib.codetr_jpeg_encode_u8(*a.values())

    for key in ("buf", "images", "out", "lengths", "ws"):
        assert call(**{key: None}) == -1, key
    assert call(N=0) == -1 and call(buf_bytes=0) == -1 and call(stride=0) == -1
    assert call(quality=0) == -1 and call(quality=101) == -1 and call(sub=2) == -1 and call(sub=-1) == -1
    assert call(N=33) == -3
    assert call(buf_bytes=1000 + 9 * 17 * 3 - 1) == -1                                    # the second image ends outside
    assert call(images=(ctypes.c_int64 * 6)(-1, 16, 16, 1000, 9, 17)) == -1
    assert call(images=(ctypes.c_int64 * 6)(1, 0, 16, 1000, 9, 17)) == -1
    assert call(images=(ctypes.c_int64 * 6)(1, 16385, 1, 1000, 9, 17), buf_bytes=1 << 30) == -3
    assert call(ws_bytes=need - 1) == -1 and call(ws=ctypes.c_void_p((1 << 21) + 8)) == -1   # too small, misaligned


# ---- 6. settings --------------------------------------------------------------------------------------------------------------
def test_vis_format_settings():
    from codetr.inferencer import vis_format_settings

    assert vis_format_settings(None) is None and vis_format_settings("png") is None
    assert vis_format_settings(dict(type="png")) is None
    assert vis_format_settings("jpeg") == dict(quality=90, subsampling="420")
    assert vis_format_settings(dict(type="jpeg")) == dict(quality=90, subsampling="420")
    assert vis_format_settings(dict(type="jpeg", quality=75, subsampling="444")) == dict(quality=75, subsampling="444")
    assert vis_format_settings(dict(quality=100.0)) == dict(quality=100, subsampling="420")
    for bad in ("jpg", 3, dict(type="webp"), dict(type="jpeg", qualty=90), dict(type="jpeg", quality=0),
                dict(type="jpeg", quality=101), dict(type="jpeg", quality=90.5), dict(type="jpeg", quality=True),
                dict(type="jpeg", quality="90"), dict(type="jpeg", subsampling="422"), dict(type="jpeg", subsampling=420),
                dict(type="png", quality=90)):
        with pytest.raises(ValueError):
            vis_format_settings(bad)


def test_inferencer_takes_vis_format():
    from codetr.inferencer import Inferencer
    from test_inferencer_batch_gpu import SWIN

    assert Inferencer(None, SWIN, None).vis_format is None
    assert Inferencer(None, SWIN, None, vis_format="png").vis_format is None
    inf = Inferencer(None, SWIN, None, visualizer=dict(), vis_format=dict(type="jpeg", quality=80))
    assert inf.vis_format == dict(quality=80, subsampling="420")
    with pytest.raises(ValueError):
        Inferencer(None, SWIN, None, vis_format=dict(type="jpeg", quality=0))
    with pytest.raises(ValueError, match="vis_format"):   # return_vis="jpeg" without the option; raised before any GPU work
        Inferencer(None, SWIN, None, visualizer=dict())([np.zeros((8, 8, 3), np.uint8)], return_vis="jpeg")


def test_encode_jpeg_rejects_bad_arguments_before_the_gpu():
    import torch

    from codetr import hip_ops

    with pytest.raises(ValueError, match="GPU"):
        hip_ops.encode_jpeg(torch.zeros(192, dtype=torch.uint8), [(0, 8, 8)])
    with pytest.raises(ValueError, match="quality"):
        hip_ops.encode_jpeg(torch.zeros(192, dtype=torch.uint8), [(0, 8, 8)], quality=0)
    assert hip_ops.jpeg_out_stride([(0, 1080, 1920)]) == (1080 * 1920 * 3 // 8 + 4096 + 15) // 16 * 16
    assert hip_ops.jpeg_out_stride([(0, 1, 1), (3, 8, 8)], "444") == 1248        # the bound of one block row: 3 * 416
