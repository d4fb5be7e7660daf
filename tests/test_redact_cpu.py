"""CPU: the numpy restatement of the redaction rule (tests/redact_ref.py, include/codetr_redact.h) against its own
invariants on the cases of tests/redact_cases.py, and what of the host side runs without a GPU: the settings, the
Inferencer's argument, the binding's table against the header, the launcher's argument checks."""
import ctypes
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import redact_cases as cases
import redact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIN = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")
MODES, SHAPES = ("pixelate", "blur", "fill"), ("box", "ellipse")


@functools.lru_cache(maxsize=None)
def _images():
    buf, rows = cases.buffer(cases.SIZES, 7)
    buf.setflags(write=False)
    return buf, rows


def _image(n):
    buf, rows = _images()
    off, H, W = rows[n]
    return buf[off:off + H * W * 3].reshape(H, W, 3)


def test_the_cases_take_every_branch():
    for H, W in cases.SIZES:
        boxes, scores, labels, count, names = cases.mix(H, W)
        rows = R.selected_rows(boxes, scores, labels, count, cases.THR, cases.SELECT)
        got = [names[j] for j in rows]
        assert got == ["overlap_a", "overlap_b", "tile_corner", "partly_outside", "wholly_outside", "zero_width",
                       "bottom_right", "small"]
        regs = {names[j]: R.region(boxes[j], 0.1) for j in rows}
        x1, y1, x2, y2 = regs["wholly_outside"]
        assert x1 >= W and y1 >= H and not R.region_mask(H, W, regs["wholly_outside"], "box").any()
        a, b = R.region_mask(H, W, regs["overlap_a"], "box"), R.region_mask(H, W, regs["overlap_b"], "box")
        assert (a & b).any()
        m = R.region_mask(H, W, regs["partly_outside"], "box")
        assert m[0, 0] and regs["partly_outside"][0] < 0
    # zero width: X2 = ceil(x) - 1 is floor(x) for a fractional x, one column; no region for a whole x
    assert R.region((10.5, 2.0, 10.5, 9.0), 0.5) == (10, -2, 10, 12) and R.region((10.0, 2.0, 10.0, 9.0), 0.5) is None
    assert R.region((10.5, 2.0, 10.5, 9.0), 0.0) == (10, 2, 10, 8)
    assert R.region((3.0, 4.0, 2.0, 9.0), 0.0) is None
    assert R.region((-1e9, -1e9, 1e9, 1e9), 1.0) == (-16384, -16384, 16382, 16382)
    # the tile corner of the 70 x 131 image lies inside the third region
    H, W = cases.SIZES[0]
    assert R.region_mask(H, W, R.region(cases.mix(H, W)[0][2], 0.0), "box")[63:65, 63:65].all()


def test_ellipse_is_inside_its_box_and_symmetric():
    reg = (3, 2, 42, 21)
    box, ell = R.region_mask(30, 50, reg, "box"), R.region_mask(30, 50, reg, "ellipse")
    assert box.sum() == 40 * 20 and 0.7 * box.sum() < ell.sum() < 0.8 * box.sum() and not (ell & ~box).any()
    inner = ell[2:22, 3:43]
    assert np.array_equal(inner, inner[::-1]) and np.array_equal(inner, inner[:, ::-1])
    assert not inner[0, 0] and inner[10, 0] and inner[0, 20]
    assert R.region_mask(5, 5, (2, 2, 2, 2), "ellipse").sum() == 1          # a one-pixel region is its pixel
    # the largest terms stay below 2^60 (the header's bound), so int64 does not wrap
    Ww = Hh = 32768
    assert ((Ww - 1) * Hh) ** 2 + ((Hh - 1) * Ww) ** 2 < 2 ** 62 and (Ww * Hh) ** 2 == 2 ** 60


@pytest.mark.parametrize("mode,shape", list(itertools.product(MODES, SHAPES)))
def test_invariants(mode, shape):
    for n, (H, W) in enumerate(cases.SIZES):
        img = _image(n)
        boxes, scores, labels, count, _ = cases.mix(H, W)
        for cell in (4, 16, 64):
            st = dict(mode=mode, shape=shape, cell=cell, score_thr=cases.THR, fill=(1, 2, 3))
            m, rows = R.mask(H, W, boxes, scores, labels, count, R.settings(**st), cases.SELECT)
            out, rows2 = R.redact(img, boxes, scores, labels, st, cases.SELECT, count)
            assert rows == rows2 and m.any() and (not m.all() or (H, W) == (5, 7))
            assert np.array_equal(out[~m], img[~m])                                  # unmasked pixels are untouched
            if mode == "fill":
                assert (out[m] == (1, 2, 3)).all()
            if mode == "pixelate":
                for k in range(-(-H // cell)):
                    for i in range(-(-W // cell)):
                        sl = (slice(k * cell, (k + 1) * cell), slice(i * cell, (i + 1) * cell))
                        vals = out[sl][m[sl]]
                        assert len(vals) == 0 or (vals == vals[0]).all()             # constant per (cell, mask)
            # the order of the rows does not matter
            perm = np.random.default_rng(cell).permutation(count)
            perm = np.concatenate((perm, np.arange(count, len(boxes))))
            again, _ = R.redact(img, boxes[perm], scores[perm], labels[perm], st, cases.SELECT, count)
            assert np.array_equal(again, out)
            # count = 0: nothing
            assert np.array_equal(R.redact(img, boxes, scores, labels, st, cases.SELECT, 0)[0], img)
    if mode != "fill":   # a constant image is a fixed point
        const = np.full((70, 131, 3), (7, 130, 255), np.uint8)
        boxes, scores, labels, count, _ = cases.mix(70, 131)
        for cell in (4, 8, 16, 32, 64):
            out, _ = R.redact(const, boxes, scores, labels, dict(mode=mode, shape=shape, cell=cell), None, count)
            assert np.array_equal(out, const)


def test_means_and_tent_known_answers():
    img = np.zeros((4, 8, 3), np.uint8)
    img[:, :4] = (10, 20, 30)
    img[:, 4:] = (50, 60, 71)
    img[0, 0] = (11, 20, 30)
    means = R.cell_means(img, 4)
    assert means.shape == (1, 2, 3) and means[0, 0].tolist() == [10, 20, 30] and means[0, 1].tolist() == [50, 60, 71]
    img[0, 0] = (18, 20, 30)                      # (160 + 8 + 8) // 16 = 11
    assert R.cell_means(img, 4)[0, 0, 0] == 11
    b = R.blurred(img, 4)
    # x = 1 lies left of the first centre (2): clamped, the first mean; x = 3: u = 3, weights 5 and 3 of 8
    assert b[0, 1].tolist() == [11, 20, 30] and b[0, 3, 0] == (5 * 11 + 3 * 50) * 8 + 32 >> 6
    assert b[0, 7].tolist() == [50, 60, 71]
    clipped = R.cell_means(np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3), 4)
    assert clipped.shape == (2, 2, 3) and clipped[1, 1, 0] == (4 * 7 + 5) * 3    # one row of three pixels: its middle


def test_settings():
    from codetr import hip_ops

    assert hip_ops.REDACT == R.DEFAULTS
    assert hip_ops.redact_style() == hip_ops.REDACT and hip_ops.redact_style() is not hip_ops.REDACT
    assert hip_ops.redact_style(dict(mode="blur", cell=64, fill=[1, 2, 3.0], expand=1))["fill"] == (1, 2, 3)
    bad = dict(mode=["gaussian", None, 1], shape=["circle", 0], cell=[0, 5, 128, 16.0, "16", True], expand=[-0.1, 1.5, "a", float("nan")],
               score_thr=["0.3", None, float("nan"), True], fill=[(0, 0), (0, 0, 256), (0, 0, -1), (0, 0, 0.5), "000", 0])
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                hip_ops.redact_style({key: v})
    with pytest.raises(ValueError, match="radius"):
        hip_ops.redact_style(dict(radius=3))


def test_inferencer_argument():
    from codetr.config import Config
    from codetr.inferencer import Inferencer, redact_settings, redacted_rows, visualizer_settings

    cfg = Config.fromfile(SWIN)
    assert redact_settings(cfg, None) is None
    full = redact_settings(cfg, {})
    assert full["style"] == R.DEFAULTS and full["classes"] is None and full["select"] is None
    meta = dict(classes=["person", "face", "plate"])
    got = redact_settings(cfg, dict(classes=["plate", 0, "person"], mode="fill"), meta)
    assert got["classes"] == [0, 2] and got["select"].tolist() == [1, 0, 1] and got["style"]["mode"] == "fill"
    vis = visualizer_settings(cfg, dict(classes=["a", "b"]), meta)       # the visualiser's names come first
    assert redact_settings(cfg, dict(classes=["b"]), meta, vis)["select"].tolist() == [0, 1]
    head = redact_settings(cfg, dict(classes=["3", 5]))                   # no metadata: str(label) of the head's classes
    assert head["classes"] == [3, 5] and len(head["select"]) == int(cfg.model.get("query_head")["num_classes"])
    for bad, key in ((dict(classes=["car"]), "classes"), (dict(classes=[3]), "classes"), (dict(classes=[-1]), "classes"),
                     (dict(classes="person"), "classes"), (dict(classes=[]), "classes"), (dict(classes=[1.5]), "classes"),
                     (dict(clases=None), "clases"), (dict(cell=5), "cell"), (dict(mode="x"), "mode"),
                     (dict(shape="x"), "shape"), (dict(expand=2), "expand"), (dict(fill=1), "fill"),
                     (dict(score_thr="a"), "score_thr")):
        with pytest.raises(ValueError, match=key):
            redact_settings(cfg, bad, meta)
    with pytest.raises(ValueError):
        redact_settings(cfg, "pixelate")
    # the constructor reads it; the default stays None
    assert Inferencer(None, SWIN, None).redact is None
    inf = Inferencer(None, SWIN, meta, redact=dict(classes=["face"], score_thr=0.5))
    assert inf.redact["classes"] == [1]
    pred = dict(labels=[1, 1, 0, 1, 1], scores=[0.9, 0.5, 0.9, float("nan"), 0.6],
                bboxes=[[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, float("inf"), 1, 1]])
    assert redacted_rows(pred, inf.redact) == [0]
    assert redacted_rows(dict(labels=[], scores=[], bboxes=[]), inf.redact) == []


def test_header_and_binding():
    from codetr import _appearance, _cabi, _cheader, _redact

    text = open(os.path.join(ROOT, "include", "codetr_redact.h")).read()
    functions, defines = _cheader.parse(text)
    assert list(functions) == ["codetr_redact_abi_version", "codetr_redact_work_bytes", "codetr_redact_detections_f16",
                               "codetr_redact_detections_bf16", "codetr_redact_detections_f32"]
    assert defines == dict(CODETR_REDACT_ABI_VERSION=1, CODETR_REDACT_PIXELATE=0, CODETR_REDACT_BLUR=1, CODETR_REDACT_FILL=2,
                           CODETR_REDACT_BOX=0, CODETR_REDACT_ELLIPSE=1, CODETR_REDACT_TILE=64)
    assert set(_redact.SIGNATURES) == set(functions) and _redact.ABI_VERSION == 1
    assert _redact.MODES == dict(pixelate=0, blur=1, fill=2) and _redact.SHAPES == dict(box=0, ellipse=1)
    i, l, p, u, f = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    assert _redact.SIGNATURES["codetr_redact_abi_version"] == (i, [])
    assert _redact.SIGNATURES["codetr_redact_work_bytes"] == (l, [l, p, l])
    for suffix in ("f16", "bf16", "f32"):
        assert _redact.SIGNATURES["codetr_redact_detections_" + suffix] == (
            i, [p, p, l, l, p, p, p, p, p, l, p, l, i, i, i, f, f, u, p, l])
    assert not set(functions) & (set(_cabi.SIGNATURES) | set(_appearance.SIGNATURES))   # a companion: the others are untouched
    assert _cabi.ABI_VERSION == 54 and _appearance.ABI_VERSION == 1
    text = " ".join(text.replace("\n *", " ").split())
    for phrase in ("parity with OpenCV's blur is unpinned", "(sum + n / 2) / n", "no term exceeds 2^60",
                   "An unmasked pixel is never written", "(strict; a NaN score fails)", ">> (2 log2 c + 2)",
                   "X2 = (int)ceilf(a2) - 1", "ex = expand * w"):
        assert phrase in text, phrase


def test_argument_checks_return_before_any_hip_call():
    """the launcher's checks are host code (csrc/redact_args.h): every rejected call returns its code without a GPU"""
    from codetr import _redact

    lib = _redact.load()
    rows = (ctypes.c_int64 * 6)(1, 70, 131, 1 + 70 * 131 * 3 + 3, 5, 7)
    assert lib.codetr_redact_abi_version() == 1
    assert lib.codetr_redact_work_bytes(2, rows, 16) == 4 * (5 * 9 + 1) == _redact.work_bytes([(1, 70, 131), (0, 5, 7)], 16)
    assert lib.codetr_redact_work_bytes(2, rows, 64) == 4 * (2 * 3 + 1) and lib.codetr_redact_work_bytes(2, rows, 4) == 4 * (18 * 33 + 4)
    assert lib.codetr_redact_work_bytes(2, rows, 5) == -1 and lib.codetr_redact_work_bytes(0, rows, 16) == -1
    assert lib.codetr_redact_work_bytes(2, None, 16) == -1 and lib.codetr_redact_work_bytes(33, rows, 16) == -3
    assert lib.codetr_redact_work_bytes(1, (ctypes.c_int64 * 3)(0, 16385, 4), 16) == -3
    assert lib.codetr_redact_work_bytes(1, (ctypes.c_int64 * 3)(0, 0, 4), 16) == -1
    one = ctypes.c_void_p(16)
    size = 1 + 70 * 131 * 3 + 3 + 5 * 7 * 3
    good = dict(stream=None, buf=one, bytes=size, N=2, rows=rows, boxes=one, scores=one, labels=one, count=one, Q=16,
                select=None, C=0, mode=0, shape=0, cell=16, thr=0.3, expand=0.1, fill=0, work=None, work_bytes=0)

    def call(**kw):
        return lib.codetr_redact_detections_f16(*dict(good, **kw).values())

    for kw, code in ((dict(buf=None), -1), (dict(rows=None), -1), (dict(boxes=None), -1), (dict(scores=None), -1),
                     (dict(labels=None), -1), (dict(count=None), -1), (dict(N=0), -1), (dict(Q=0), -1), (dict(bytes=0), -1),
                     (dict(select=one, C=0), -1), (dict(mode=3), -1), (dict(mode=-1), -1), (dict(shape=2), -1),
                     (dict(cell=0), -1), (dict(cell=24), -1), (dict(cell=128), -1), (dict(thr=float("nan")), -1),
                     (dict(expand=-0.5), -1), (dict(expand=1.5), -1), (dict(expand=float("nan")), -1),
                     (dict(fill=0x1000000), -1), (dict(bytes=size - 1), -1),                       # a row outside the buffer
                     (dict(rows=(ctypes.c_int64 * 6)(1, 70, 131, 100, 5, 7)), -1),                 # overlapping images
                     (dict(rows=(ctypes.c_int64 * 6)(-1, 70, 131, 30000, 5, 7)), -1),
                     (dict(mode=1), -1), (dict(mode=1, work=one, work_bytes=4 * 46 - 1), -1),      # blur: the workspace
                     (dict(mode=1, work=ctypes.c_void_p(18), work_bytes=4096), -1),
                     (dict(N=33), -3), (dict(Q=4097), -3), (dict(select=one, C=65537), -3),
                     (dict(N=1, rows=(ctypes.c_int64 * 3)(0, 1, 16385), bytes=1 << 20), -3)):
        assert call(**kw) == code, kw


def test_host_check_of_the_argument_checks(tmp_path):
    """csrc/redact_args.h in a stand-alone program (tests/cabi_c/redact_host_check.cpp) under
    -fsanitize=address,undefined, nothing preloaded: image tables of exactly the size a call may read"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "redact_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "redact_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:
        # a compiler without the sanitizer runtimes, or a process environment in which they cannot start: the same
        # program without them still holds every answer
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("clean"), r.stdout[-2000:] + r.stderr[-2000:]
