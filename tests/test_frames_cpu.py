"""CPU: the frame-conversion contract of include/codetr_hip.h ("Frames") -- the header's constants, known answers worked
in Python integers, the numpy reference tests/frames_ref.py, the argument contract of codetr_frames_to_rgb_u8 (every
rejection happens on the host before any HIP call) and the Inferencer's `frame_settings` / `parse_frame`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_TOO_LARGE = -1, -3
COMBOS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]


def _header_sets():
    text = open(os.path.join(ROOT, "include", "codetr_hip.h")).read()
    found = re.findall(r"#define CODETR_YUV_(BT601|BT709)_(LIMITED|FULL)\s*\{([^}]*)\}", text)
    return {(m.lower(), r.lower()): tuple(int(v) for v in body.split(",")) for m, r, body in found}


def _int_coefficients(matrix, range_):
    """round(k * 2^20), recomputed here: from the five decimals for BT.601 limited, from (Kr, Kb) otherwise"""
    if (matrix, range_) == ("bt601", "limited"):
        k = [1.164, 1.596, -0.391, -0.813, 2.018]
    else:
        kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
        kg = 1 - kr - kb
        k = [1.0, 2 * (1 - kr), -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg, 2 * (1 - kb)]
        if range_ == "limited":
            k = [k[0] * 255 / 219] + [c * 255 / 224 for c in k[1:]]
    return [round(c * 2 ** 20) for c in k]


def _raw(Y, U, V, matrix, range_):
    """the three sums before the clamp, in Python integers"""
    cy, crv, cgu, cgv, cbu = _int_coefficients(matrix, range_)
    c, d, e = max(0, Y - (16 if range_ == "limited" else 0)), U - 128, V - 128
    return ((cy * c + crv * e + (1 << 19)) >> 20, (cy * c + cgu * d + cgv * e + (1 << 19)) >> 20,
            (cy * c + cbu * d + (1 << 19)) >> 20)


def _convert(Y, U, V, matrix, range_):
    return tuple(min(255, max(0, v)) for v in _raw(Y, U, V, matrix, range_))


def test_header_literals_are_the_rounded_coefficients():
    sets = _header_sets()
    assert sorted(sets) == sorted(COMBOS)
    assert sets[("bt601", "limited")] == (1220542, 1673527, -409993, -852492, 2116026)
    for combo in COMBOS:
        assert list(sets[combo]) == _int_coefficients(*combo), combo
        assert sets[combo] + (16 if combo[1] == "limited" else 0,) == R.coefficients(*combo)
    text = open(os.path.join(ROOT, "include", "codetr_hip.h")).read()
    for name, code in list(R.FORMATS.items()) + [("max_side", 32767)]:
        assert re.search(r"#define CODETR_FRAME_%s %d\n" % (name.upper(), code), text), name
    for name, code in (("BT601", 0), ("BT709", 1), ("LIMITED", 0), ("FULL", 1)):
        assert re.search(r"#define CODETR_COLOR_%s %d\n" % (name, code), text), name
    assert "unpinned" in text[text.index("codetr_frames_to_rgb_u8"):]


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_known_answers(matrix):
    assert _convert(16, 128, 128, matrix, "limited") == (0, 0, 0)
    assert _convert(235, 128, 128, matrix, "limited") == (255, 255, 255)
    assert _convert(0, 128, 128, matrix, "full") == (0, 0, 0)
    assert _convert(255, 128, 128, matrix, "full") == (255, 255, 255)
    assert _convert(0, 128, 128, matrix, "limited") == (0, 0, 0)            # c = max(0, Y - 16)
    for range_ in ("limited", "full"):
        # saturated red, green, blue: each clamps one channel at 255 and another at 0
        for yuv, top, bottom in (((90, 0, 255), 0, 2), ((200, 0, 0), 1, 2), ((90, 255, 0), 2, 0)):
            raw = _raw(*yuv, matrix, range_)
            assert raw[top] > 255 and raw[bottom] < 0, (yuv, raw)
            got = _convert(*yuv, matrix, range_)
            assert got[top] == 255 and got[bottom] == 0
            assert tuple(R.yuv_to_rgb(*yuv, matrix, range_).tolist()) == got
        for yuv in ((16, 128, 128), (235, 128, 128), (0, 128, 128), (255, 128, 128), (128, 1, 254), (17, 129, 127)):
            assert tuple(R.yuv_to_rgb(*yuv, matrix, range_).tolist()) == _convert(*yuv, matrix, range_)
    # the largest magnitude of any sum stays below 2^30
    for range_ in ("limited", "full"):
        cy, crv, cgu, cgv, cbu = _int_coefficients(matrix, range_)
        assert cy * 255 + max(abs(crv), abs(cbu), abs(cgu) + abs(cgv)) * 128 + (1 << 19) < 1 << 30


@pytest.mark.parametrize("fmt", ["nv12", "nv21", "i420"])
def test_chroma_indexing_on_a_3x5_frame(fmt):
    H, W = 3, 5
    planes = R.random_planes(fmt, H, W, np.random.default_rng(3))
    assert [p.shape for p in planes] == ([(3, 5), (2, 6)] if fmt != "i420" else [(3, 5), (2, 3), (2, 3)])
    got = R.planes_to_rgb(fmt, H, W, planes, "bt709", "full")
    for y in range(H):
        for x in range(W):
            if fmt == "i420":
                U, V = planes[1][y >> 1, x >> 1], planes[2][y >> 1, x >> 1]
            else:
                a, b = planes[1][y >> 1, 2 * (x >> 1)], planes[1][y >> 1, 2 * (x >> 1) + 1]
                U, V = (a, b) if fmt == "nv12" else (b, a)
            assert tuple(got[y, x].tolist()) == _convert(int(planes[0][y, x]), int(U), int(V), "bt709", "full"), (y, x)
    assert np.array_equal(R.to_rgb(R.item(fmt, H, W, planes), fmt, "bt709", "full"), got)


def test_packed_formats_are_permutations():
    rng = np.random.default_rng(4)
    H, W = 3, 5
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
    assert np.array_equal(R.to_rgb(rgb, "rgb"), rgb)
    assert np.array_equal(R.to_rgb(rgb[..., ::-1], "bgr"), rgb)
    assert np.array_equal(R.to_rgb(np.concatenate((rgb, alpha), 2), "rgba"), rgb)
    assert np.array_equal(R.to_rgb(np.concatenate((rgb[..., ::-1], alpha), 2), "bgra"), rgb)
    gray = rgb[..., 0]
    assert np.array_equal(R.to_rgb(gray, "gray"), np.stack((gray,) * 3, -1))       # no range expansion
    # the 2-D array decoders hand out and the tuple of planes are the same frame
    for fmt in ("nv12", "nv21", "i420"):
        planes = R.random_planes(fmt, 4, 6, rng)
        a, b = R.item(fmt, 4, 6, planes, True), R.item(fmt, 4, 6, planes, False)
        assert a.shape == (6, 6) and isinstance(b, tuple)
        assert np.array_equal(R.to_rgb(a, fmt), R.to_rgb(b, fmt))


def test_pack_lays_planes_out_as_the_rows_say():
    rng = np.random.default_rng(5)
    frames = [(f, 3, 5, R.random_planes(f, 3, 5, rng)) for f in ("nv12", "i420", "bgr")]
    buf, rows, dst_bytes = R.pack(frames, pad=3, fill=0xA5, start=1, residues=[1, 2, 3, 0], dst_residues=[3, 0, 1])
    assert [r[3] % 4 for r in rows] == [1, 3, 2] and [r[9] % 4 for r in rows] == [3, 0, 1]
    last = rows[-1]
    assert last[3] + 2 * last[4] + 15 == buf.size                    # flush with the end of the buffer
    for (fmt, H, W, planes), row in zip(frames, rows):
        for k, a in enumerate(planes):
            off, pitch = row[3 + 2 * k], row[4 + 2 * k]
            assert pitch == a.shape[1] + 3
            for r in range(a.shape[0]):
                assert np.array_equal(buf[off + r * pitch:off + r * pitch + a.shape[1]], a[r])
    out = R.expected_output(frames, rows, dst_bytes + 7, 0x5A)
    assert out[:3].tolist() == [0x5A] * 3 and out[-7:].tolist() == [0x5A] * 7


# ---- the argument contract ----------------------------------------------------------------------------------------
@pytest.fixture
def lib():
    from codetr import _cabi

    _cabi.RECORDER = []
    try:
        yield _cabi.load()
        assert _cabi.RECORDER == []   # no rejected call reached a launch
    finally:
        _cabi.RECORDER = None


def _table(rows):
    return (ctypes.c_int64 * (10 * len(rows)))(*[v for r in rows for v in r])


def test_frames_to_rgb_rejects_bad_arguments(lib):
    from codetr import _cabi

    assert _cabi.FRAME_FORMATS == R.FORMATS and _cabi.FRAME_MAX_SIDE == 32767
    assert _cabi.COLOR_MATRICES == R.MATRICES and _cabi.COLOR_RANGES == R.RANGES
    f = lib.codetr_frames_to_rgb_u8
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    # a 4 x 6 NV12 frame with pitches 8: Y rows end at 24 + 6 = 30 <= 32, UV (2 rows of 6) at 32, ends at 32 + 8 + 6 = 46
    nv12 = (5, 4, 6, 0, 8, 32, 8, 0, 0, 0)
    ok = dict(src=one, nbytes=46, N=1, tab=_table([nv12]), matrix=0, range=0, dst=one, dbytes=72)

    def call(**kw):
        a = dict(ok, **kw)
        return f(None, a["src"], a["nbytes"], a["N"], a["tab"], a["matrix"], a["range"], a["dst"], a["dbytes"])

    def row(**kw):
        names = ("fmt", "H", "W", "off0", "pitch0", "off1", "pitch1", "off2", "pitch2", "dst")
        r = dict(zip(names, kw.pop("base", nv12)))
        r.update(kw)
        return _table([tuple(r[k] for k in names)])

    assert call(src=None) == E_BADARG
    assert call(tab=None) == E_BADARG
    assert call(dst=None) == E_BADARG
    assert call(N=0) == E_BADARG and call(N=-1) == E_BADARG
    assert call(nbytes=0) == E_BADARG and call(dbytes=0) == E_BADARG
    assert call(tab=row(fmt=8)) == E_BADARG and call(tab=row(fmt=-1)) == E_BADARG
    assert call(matrix=2) == E_BADARG and call(matrix=-1) == E_BADARG
    assert call(range=2) == E_BADARG and call(range=-1) == E_BADARG
    assert call(tab=row(H=0)) == E_BADARG and call(tab=row(W=0)) == E_BADARG and call(tab=row(H=-4)) == E_BADARG
    for col in ("off0", "off1", "off2", "dst"):
        assert call(tab=row(**{col: -1})) == E_BADARG, col
    assert call(tab=row(pitch0=5)) == E_BADARG                      # a pitch smaller than the row's bytes
    assert call(tab=row(pitch1=5)) == E_BADARG
    assert call(nbytes=45) == E_BADARG                               # the last chroma row ends one byte past src_bytes
    assert call(tab=row(off1=33)) == E_BADARG
    assert call(tab=row(off0=27, off1=0), nbytes=46) == E_BADARG     # the last Y row ends one byte past src_bytes
    assert call(dbytes=71) == E_BADARG                               # the output image does not lie inside dst
    assert call(tab=row(dst=1)) == E_BADARG
    assert call(tab=row(pitch0=1 << 62)) == E_BADARG                 # (no overflow in the row arithmetic)
    two = [nv12, nv12[:9] + (71,)]
    assert call(N=2, tab=_table(two), dbytes=200) == E_BADARG        # two output images overlap by one byte
    assert call(N=2, tab=_table([nv12[:9] + (10,), nv12]), dbytes=200) == E_BADARG   # ... whichever comes first
    assert call(N=2, tab=_table([nv12, nv12[:9] + (72,)]), dbytes=143) == E_BADARG   # the second one past dst
    assert call(N=33, tab=_table([nv12] * 33)) == E_TOO_LARGE
    assert call(tab=row(H=32768), nbytes=1 << 40, dbytes=1 << 40) == E_TOO_LARGE
    assert call(tab=row(W=32768, pitch0=32768, pitch1=32768), nbytes=1 << 40, dbytes=1 << 40) == E_TOO_LARGE
    # every plane of every format is bounded: the last row of the last plane one byte short
    for fmt, H, W in [(f, h, w) for f in R.FORMATS for h, w in ((3, 5), (4, 6))]:
        planes = R.random_planes(fmt, H, W, np.random.default_rng(0))
        buf, rows, dst_bytes = R.pack([(fmt, H, W, planes)], pad=2)
        assert call(tab=_table(rows), nbytes=buf.size - 1, dbytes=dst_bytes) == E_BADARG, fmt
        assert call(tab=_table(rows), nbytes=buf.size, dbytes=dst_bytes - 1) == E_BADARG, fmt
        k = len(planes) - 1
        short = list(rows[0])
        short[4 + 2 * k] = planes[k].shape[1] - 1
        assert call(tab=_table([tuple(short)]), nbytes=buf.size, dbytes=dst_bytes) == E_BADARG, fmt


# ---- the Inferencer's settings and item parser -------------------------------------------------------------------
def test_frame_settings():
    from codetr.inferencer import frame_settings

    assert frame_settings() == dict(format="rgb", matrix="bt601", range="limited")
    assert frame_settings("nv12", dict(range="full")) == dict(format="nv12", matrix="bt601", range="full")
    assert frame_settings("i420", dict(matrix="bt709")) == dict(format="i420", matrix="bt709", range="limited")
    for name in R.FORMATS:
        assert frame_settings(name)["format"] == name
    with pytest.raises(ValueError, match="input_format must be one of"):
        frame_settings("yuyv")
    with pytest.raises(ValueError, match="input_format must be one of"):
        frame_settings(5)
    with pytest.raises(ValueError, match="color must be None or a dict"):
        frame_settings("nv12", dict(primaries="bt709"))
    with pytest.raises(ValueError, match="color must be None or a dict"):
        frame_settings("nv12", "bt709")
    with pytest.raises(ValueError, match="color matrix"):
        frame_settings("nv12", dict(matrix="bt2020"))
    with pytest.raises(ValueError, match="color range"):
        frame_settings("nv12", dict(range="tv"))


def test_parse_frame_accepts_every_documented_shape():
    from codetr.inferencer import parse_frame

    rng = np.random.default_rng(6)
    for fmt, (H, W) in [(f, s) for f in R.FORMATS for s in ((3, 5), (4, 6))]:
        planes = R.random_planes(fmt, H, W, rng)
        items = [R.item(fmt, H, W, planes)]
        if fmt in ("nv12", "nv21", "i420"):
            items.append(R.item(fmt, H, W, planes, False))
        items += [torch.from_numpy(np.ascontiguousarray(i)) if not isinstance(i, tuple)
                  else tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in i) for i in list(items)]
        for it in items:
            fr = parse_frame(it, fmt)
            assert (fr.code, fr.H, fr.W, fr.resident) == (R.FORMATS[fmt], H, W, False)
            assert [p.shape for p in fr.planes] == R.plane_shapes(fmt, H, W)
            assert all(np.array_equal(a, b) for a, b in zip(fr.planes, planes)), fmt
    # a strided host view: the rows of a wider surface
    wide = rng.integers(0, 256, (6, 16), dtype=np.uint8)
    fr = parse_frame(wide[:, 3:9], "nv12")
    assert (fr.H, fr.W) == (4, 6) and np.array_equal(fr.planes[1], wide[4:, 3:9])
    fr = parse_frame(wide[:, 3:9], "i420")   # (two chroma rows per array row: copied, then split)
    assert np.array_equal(np.concatenate([p.reshape(-1) for p in fr.planes]), wide[:, 3:9].reshape(-1))


def test_parse_frame_rejections_name_the_format():
    from codetr.inferencer import parse_frame

    z = np.zeros
    cases = [
        ("rgb", z((4, 6), np.uint8), "got shape"), ("rgb", z((4, 6, 4), np.uint8), "got shape"),
        ("bgr", z((4, 6, 3), np.float32), "float32"), ("bgr", [[1, 2, 3]], "tuple of planes"),
        ("rgba", z((4, 6, 3), np.uint8), "got shape"), ("bgra", "frame.png", "got str"),
        ("gray", z((4, 6, 1), np.uint8), "got shape"), ("gray", z((0, 6), np.uint8), "got shape"),
        ("nv12", z((5, 6), np.uint8), "got shape"),            # rows not a multiple of 3
        ("nv12", z((6, 5), np.uint8), "got shape"),            # odd W as a 2-D array
        ("nv12", z((4, 6, 3), np.uint8), "got shape"),
        ("nv12", (z((3, 5), np.uint8),), "1 plane"),
        ("nv12", (z((3, 5), np.uint8), z((2, 3), np.uint8)), "chroma plane of shape"),
        ("nv21", (z((3, 5), np.uint8), z((1, 3, 2), np.uint8)), "chroma plane of shape"),
        ("i420", (z((3, 5), np.uint8), z((2, 3), np.uint8)), "2 plane"),
        ("i420", (z((3, 5), np.uint8), z((2, 3), np.uint8), z((2, 2), np.uint8)), "chroma plane of shape"),
        ("i420", torch.zeros((6, 6), dtype=torch.float16), "float16"),
    ]
    assert parse_frame(z((3, 6), np.uint8), "nv21")[1:3] == (2, 6)      # the smallest 2-D frame
    for fmt, item, why in cases:
        with pytest.raises(ValueError, match=why) as e:
            parse_frame(item, fmt)
        assert f"input_format={fmt!r}" in str(e.value), (fmt, str(e.value))


def test_host_rgb_tells_the_reference_route_from_the_staged_one():
    from codetr.inferencer import Inferencer

    assert Inferencer.host_rgb([np.zeros((2, 2, 3), np.uint8)]) and Inferencer.host_rgb([], None)
    assert not Inferencer.host_rgb([torch.zeros((2, 2, 3), dtype=torch.uint8)])
    assert not Inferencer.host_rgb([np.zeros((2, 2, 3), np.uint8)], dict(format="bgr"))
