"""CPU: the JPEG decoder's rule and its host parts.  The numpy restatement of include/codetr_jpeg_dec.h
(tests/jpeg_dec_ref.py) is held to Pillow exactly; the library's host-only parser to the restatement's, on the committed
files, on every prefix and every single-byte change of a header; the chunked fixed point to the sequential decode; and
the decoder core the kernels call is run on the host, stand-alone, under the address and undefined-behaviour sanitizers
(tests/cabi_c/jpeg_dec_host_check.cpp) over every file, the corrupt scans of the GPU tests and seeded corruptions."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_dec_cases as C
import jpeg_dec_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------
def test_restatement_equals_pillow_on_the_committed_files():
    for name in C.SUPPORTED:
        rgb, status, _ = C.expected(name)
        assert status == 0, name
        assert np.array_equal(rgb, _pillow(C.data(name))), name


def test_restatement_equals_pillow_on_generated_files():
    """H in {1, 2, 3, 5, 9, 16, 17, 18, 31} x W in {1..7, 15, 16, 17, 33}, 4:2:2 and 4:2:0, with and without restart
    markers: replication for dw <= 2, the fancy rule above, odd sizes at every edge"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    for H in (1, 2, 3, 5, 9, 16, 17, 18, 31):
        for W in (1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 33):
            arr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            for sub in (1, 2):
                for kw in ({}, dict(restart_marker_blocks=2)):
                    f = io.BytesIO()
                    Image.fromarray(arr).save(f, "JPEG", quality=92, subsampling=sub, **kw)
                    rgb, status = D.decode(f.getvalue())
                    assert status == 0 and np.array_equal(rgb, _pillow(f.getvalue())), (H, W, sub, kw)


def test_restatement_round_trips_the_projects_encoder():
    import jpeg_ref

    f = C.encoder_file()
    info = D.parse(f)
    assert (info["H"], info["W"], info["dri"], info["hmax"], info["vmax"]) == (160, 40, 3, 2, 2)
    coef, status = D.decode_coefficients(info, D.scan_of(f, info))
    assert status == 0
    # exactly the coefficients the encoder's restatement quantised, block for block in MCU order
    y, cb, cr = jpeg_ref.ycc_planes(C.encoder_image(), "420")
    qy = jpeg_ref.quantised_blocks(y, jpeg_ref.quant_table(90, jpeg_ref.BASE_LUM))
    qc = [jpeg_ref.quantised_blocks(p, jpeg_ref.quant_table(90, jpeg_ref.BASE_CHROM)) for p in (cb, cr)]
    want = []
    for my in range(info["mcus_y"]):
        for mx in range(info["mcus_x"]):
            want += [qy[2 * my + v, 2 * mx + h] for v in (0, 1) for h in (0, 1)] + [qc[0][my, mx], qc[1][my, mx]]
    natural = np.zeros((len(want), 64), np.int64)
    natural[:, D.ZIGZAG] = np.stack(want)
    assert np.array_equal(coef, natural)
    rgb = D.pixels(info, coef)
    assert rgb.shape == (160, 40, 3) and np.array_equal(rgb, D.decode(f)[0])
    try:
        assert np.array_equal(rgb, _pillow(f))
    except pytest.skip.Exception:
        pass


def test_chunked_fixed_point_equals_the_sequential_decode():
    for name in (C.NOISE, C.GRADIENT):
        raw = C.data(name)
        info = D.parse(raw)
        scan = D.scan_of(raw, info)
        stats = {}
        coef, status = D.decode_chunked(info, scan, stats=stats)
        want, want_status = D.decode_coefficients(info, scan)
        assert status == want_status == 0 and np.array_equal(coef, want), name
        assert stats["chunks"] > D.RUN and max(stats["rounds"]) <= D.RUN, (name, stats["rounds"])
        if name == C.NOISE:   # no restart markers, dense data: dozens of rounds, and runs whose guessed entry was wrong
            assert max(stats["rounds"]) >= 20 and stats["repaired"], stats


def test_case_list_coverage():
    """the committed files reach every path of the entropy decoder and the upsampler"""
    total = {}
    for name in C.SUPPORTED:
        for k, v in C.expected(name)[2].items():
            total[k] = max(total.get(k, 0), v)
    assert total["zrl"] > 0 and total["no_eob"] > 0 and total["max_dc_category"] >= 10
    stuffed = straddles = after_rst = 0
    for name in C.SUPPORTED:
        raw = C.data(name)
        info = D.parse(raw)
        scan = D.scan_of(raw, info)
        for i in range(len(scan) - 1):
            if scan[i] == 0xFF and scan[i + 1] == 0:
                stuffed += 1
                straddles += (i + 1) % D.CHUNK == 0            # a chunk boundary between an FF and its 00
            if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
                after_rst += (i + 2) % D.CHUNK == 0            # a chunk that begins right after an RSTm
    assert stuffed > 0 and straddles > 0 and after_rst > 0, (stuffed, straddles, after_rst)
    small = [D.parse(C.data(n)) for n in C.SUPPORTED]
    assert any(i["hmax"] == 2 and -(-i["W"] // 2) <= 2 for i in small)          # dw <= 2: replication
    assert any(i["hmax"] == 2 and i["vmax"] == 2 and -(-i["W"] // 2) == 3 for i in small)   # the smallest fancy case
    assert {(i["ncomp"], i["hmax"], i["vmax"]) for i in small} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert any(i["dri"] for i in small) and any(not i["dri"] for i in small)
    assert all(C.expected(n)[1] != 0 for n in C.corrupt())
    assert len({C.expected(n)[1] for n in C.corrupt()}) >= 3


# ---- 2. the header and the binding ----------------------------------------------------------------------------------------
def test_header_constants_and_version():
    from codetr import _cabi, _jpeg, _jpeg_dec

    assert _jpeg_dec.ABI_VERSION == 1 and _jpeg_dec.load().codetr_jpegdec_abi_version() == 1
    assert _jpeg.ABI_VERSION == 1 and _cabi.ABI_VERSION == 54                  # the other headers are untouched
    assert sorted(_jpeg_dec.functions) == ["codetr_jpegdec_abi_version", "codetr_jpegdec_decode_u8", "codetr_jpegdec_output_bytes",
                                           "codetr_jpegdec_parse", "codetr_jpegdec_workspace_bytes"]
    assert _jpeg_dec.functions["codetr_jpegdec_decode_u8"][1][0] == ("void *", "stream")
    assert (_jpeg_dec.CHUNK_BYTES, _jpeg_dec.RUN_CHUNKS) == (D.CHUNK, D.RUN)
    assert _jpeg_dec.TABLE_BYTES == 4 * 64 + 8 * (16 + 256) and _jpeg_dec.MAX_FILE_BYTES == D.MAX_FILE
    assert _jpeg_dec.REASONS == {i: n for i, n in enumerate(D.REASONS) if n}
    assert _jpeg_dec.STATUS == {i: n for i, n in enumerate(D.STATUS) if i}
    assert "jpeg_decode" in _cabi.CALLS
    text = open(_jpeg_dec.HEADER_PATH).read()
    for constant in (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172, 91881, 22554, 46802, 116130):
        assert str(constant) in text, constant
    assert _jpeg_dec.output_bytes(3, 5) == 48 and _jpeg_dec.output_bytes(1, 1) == 16
    with pytest.raises(RuntimeError):
        _jpeg_dec.output_bytes(0, 5)


def _c_parse(raw):
    from codetr import _jpeg_dec

    return _jpeg_dec.parse(np.frombuffer(raw, np.uint8) if len(raw) else np.zeros(0, np.uint8))


def _ref_code(raw):
    try:
        return 0, 0, D.parse(raw)
    except D.ParseError as e:
        return e.code, e.reason, e.info


def test_parser_matches_the_files():
    from codetr import hip_ops

    for name in C.SUPPORTED:
        raw = C.data(name)
        rc, info, tables = _c_parse(raw)
        ref = D.parse(raw)
        assert rc == 0 and info[6] == 0, name
        assert (info[0], info[1], info[2], info[3], info[4], info[5]) == (ref["H"], ref["W"], ref["ncomp"], ref["dri"],
                                                                         ref["scan_offset"], ref["scan_bytes"]), name
        assert raw[info[4] + info[5]:info[4] + info[5] + 2] == b"\xff\xd9" and raw[info[4] - 3:info[4]] == b"\x00\x3f\x00"
        assert (info[7], info[8], info[24], info[25], info[26], info[27]) == (ref["hmax"], ref["vmax"], ref["mcus_x"],
                                                                             ref["mcus_y"], ref["bpm"], ref["nblocks"])
        for c, comp in enumerate(ref["comps"]):
            assert tuple(info[9 + 5 * c:14 + 5 * c]) == comp, (name, c)
        for t in range(4):
            assert tables[64 * t:64 * t + 64].tolist() == ref["quant"].get(t, [0] * 64), (name, t)
        for cls in range(2):
            for t in range(4):
                bits, vals = ref["huff"].get((cls, t), ([0] * 16, []))
                got = tables[256 + (cls * 4 + t) * 272:256 + (cls * 4 + t + 1) * 272]
                assert got[:16].tolist() == bits and got[16:16 + len(vals)].tolist() == vals and not got[16 + len(vals):].any()
        assert hip_ops.jpeg_info(raw)["supported"] and hip_ops.jpeg_info(raw)["sampling"][0] == (ref["hmax"], ref["vmax"])
    for name, reason in C.REFUSED.items():
        rc, info, _ = _c_parse(C.data(name))
        assert rc == D.E_UNSUPPORTED and D.REASONS[info[6]] == reason, name
        assert _ref_code(C.data(name))[:2] == (D.E_UNSUPPORTED, info[6])
        got = hip_ops.jpeg_info(C.data(name))
        assert not got["supported"] and got["reason"] == reason and (got["height"], got["width"]) == (24, 24)


def test_parser_refuses_each_unsupported_kind():
    """edits of one file's header, one per reason code"""
    raw = bytearray(C.data("444_8x8_q90_opt"))
    sof, sos, dqt = raw.index(b"\xff\xc0"), raw.index(b"\xff\xda"), raw.index(b"\xff\xdb")

    def edited(at, value, insert=b""):
        out = bytearray(raw)
        if at is not None:
            out[at] = value
        return bytes(out[:2] + insert + out[2:])

    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00"
    cases = {
        "extended": edited(sof + 1, 0xC1), "lossless": edited(sof + 1, 0xC3), "hierarchical": edited(sof + 1, 0xC5),
        "arithmetic": edited(sof + 1, 0xC9), "precision": edited(sof + 4, 12), "adobe": edited(None, 0, adobe + b"\x00"),
        "rgb_ids": None, "scan_params": edited(sos + 4 + 1 + 6, 1),
    }
    ids = bytearray(raw)
    for c, ch in enumerate(b"RGB"):
        ids[sof + 10 + 3 * c] = ch
        ids[sos + 5 + 2 * c] = ch
    cases["rgb_ids"] = bytes(ids)
    q16 = bytearray(raw)
    seg = (q16[dqt + 2] << 8 | q16[dqt + 3])
    assert seg == 67
    cases["quant16"] = bytes(q16[:dqt] + b"\xff\xdb\x00\x83\x10" + bytes(128) + q16[dqt:])
    for reason, data in cases.items():
        rc, info, _ = _c_parse(data)
        assert rc == D.E_UNSUPPORTED and D.REASONS[info[6]] == reason, (reason, rc, info[6])
        assert _ref_code(data)[:2] == (rc, info[6]), reason
    assert _c_parse(edited(None, 0, adobe + b"\x01"))[0] == 0                      # transform 1 (YCbCr) is the supported one
    big = bytearray(raw)
    big[sof + 5] = 0x80
    assert _c_parse(bytes(big))[0] == D.E_TOO_LARGE == _ref_code(bytes(big))[0]


def test_parser_on_truncated_and_garbled_headers():
    """every prefix of one small file and every single-byte change of its header: E_BADARG, E_UNSUPPORTED (E_TOO_LARGE
    where the change makes a side larger than the limit), or a parse whose scan lies inside the file -- and always what
    the restatement's parser says"""
    raw = C.data("420_2x3_q90_opt")
    info = D.parse(raw)
    codes = (D.E_BADARG, D.E_UNSUPPORTED, D.E_TOO_LARGE)

    def check(data, what):
        rc, got, _ = _c_parse(data)
        want = _ref_code(data)
        assert rc == want[0] and (rc != D.E_UNSUPPORTED or got[6] == want[1]), (what, rc, want[:2])
        if rc == 0:
            assert 0 <= got[4] and 0 <= got[5] and got[4] + got[5] + 2 <= len(data), what
            assert (got[0], got[1], got[4], got[5]) == (want[2]["H"], want[2]["W"], want[2]["scan_offset"], want[2]["scan_bytes"])
        else:
            assert rc in codes, (what, rc)
        return rc

    seen = {check(raw[:n], n) for n in range(len(raw) + 1)}
    assert seen == {0, D.E_BADARG}                      # (only the whole file, and the one that ends at EOI, parse)
    seen = set()
    for at in range(info["scan_offset"]):
        for value in range(256):
            if value != raw[at]:
                seen.add(check(raw[:at] + bytes([value]) + raw[at + 1:], (at, value)))
    assert seen == {0} | set(codes)


# ---- 3. the host memory check ---------------------------------------------------------------------------------------------
def test_host_memory_check(tmp_path):
    """the parser and the core the kernels call, on the host under -fsanitize=address,undefined (a stand-alone program,
    nothing preloaded): every committed file, the GPU tests' corrupt scans and seeded corruptions; statuses and pixels
    equal the restatement's"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_dec_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "jpeg_dec_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = [exe, "--corrupt", "0", os.path.join(C.DIR, "444_1x1_q90.jpg")]
    if (subprocess.run(cmd + san, capture_output=True).returncode != 0
            or subprocess.run(probe, capture_output=True).returncode != 0):
        # a compiler without the sanitizer runtimes, or a process environment in which they cannot start: the same
        # program without them still holds statuses and pixels to the restatement
        subprocess.run(cmd, check=True, capture_output=True)
    paths = []
    for name, data in C.corrupt().items():
        (tmp_path / (name + ".jpg")).write_bytes(data)
        paths.append(str(tmp_path / (name + ".jpg")))
    small = [n for n in C.NAMES if "320x240" not in n]
    runs = ((300, [os.path.join(C.DIR, n + ".jpg") for n in small] + paths),
            (6, [os.path.join(C.DIR, n + ".jpg") for n in C.NAMES if "320x240" in n]))
    lines = {}
    for corrupt, files in runs:
        r = subprocess.run([exe, "--out", str(tmp_path), "--corrupt", str(corrupt)] + files, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("clean"), r.stdout[-2000:] + r.stderr[-2000:]
        for line in r.stdout.splitlines()[:-1]:
            lines[line.split()[0][:-4]] = line.split()
    for name in C.SUPPORTED + list(C.corrupt()):
        rgb, status, _ = C.expected(name)
        assert lines[name][1:4] == ["0", "0", str(status)], lines[name]
        got = np.fromfile(str(tmp_path / (name + ".jpg.rgb")), np.uint8).reshape(rgb.shape)
        if status == 0:
            assert np.array_equal(got, rgb), name
    for name, reason in C.REFUSED.items():
        assert lines[name][1:3] == [str(D.E_UNSUPPORTED), str(D.R[reason])]
