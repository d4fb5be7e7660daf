"""CPU: the restatement of the crop rule (tests/crops_ref.py) against the unrounded filter in float64, its sharp
properties, Pillow where it imports; the settings, the Inferencer's argument, the launcher's argument checks."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import crops_ref as R
import redact_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIN = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")
CASES = pytest.mark.parametrize("name,n,box,size", R.CASES, ids=[c[0] for c in R.CASES])
# the largest |restatement - Pillow| measured over CASES (the header and the README quote both)
PILLOW_MAX, PILLOW_CUT_MAX = 79, 1


def _case(n, box, size, fit="stretch"):
    buf, rows = redact_cases.buffer(R.SIZES, 7)
    off, H, W = rows[n]
    return (buf[off:off + H * W * 3].reshape(H, W, 3), R.region(box, 0.0, H, W),
            dict(R.DEFAULTS, size=size, fit=fit, pad_value=(9, 200, 31)))


@pytest.mark.parametrize("fit", ["stretch", "pad"])
@CASES
def test_restatement_against_the_float64_filter(name, n, box, size, fit):
    """The reference: per axis the normalised triangle weights max(0, 1 - |s + 1/2 - centre| / max(1, R / n)), applied as
    the separable 2-D sum in float64 and never rounded.  The rule rounds twice.  The row value t is hs / Nrm rounded to a
    multiple of 1/256, an error of at most 1/512 per row; the vertical weights are non-negative and sum to one, so the
    column sum inherits at most 1/512.  The final division rounds to the nearest integer: at most 1/2.  Hence
    |out - reference| <= 1/2 + 1/512 LSB (float64 evaluation error, ~1e-13, is far inside the 1e-9 added below)."""
    img, (x0, y0, x1, y1), st = _case(n, box, size, fit)
    ox, oy, iw, ih = R.inner_rect(fit, x1 - x0, y1 - y0, *size)

    def axis(n_out, length):
        centre = (np.arange(n_out)[:, None] + 0.5) * length / n_out
        wt = np.maximum(0.0, 1.0 - np.abs(np.arange(length)[None, :] + 0.5 - centre) / max(1.0, length / n_out))
        return wt / wt.sum(1, keepdims=True)

    ref = np.einsum("jy,yic->jic", axis(ih, y1 - y0), np.einsum("ix,yxc->yic", axis(iw, x1 - x0), img[y0:y1, x0:x1].astype(np.float64)))
    err = np.abs(R.crop(img, (x0, y0, x1, y1), st)[oy:oy + ih, ox:ox + iw] - ref).max()
    assert err <= 0.5 + 1.0 / 512 + 1e-9, err


@CASES
def test_identity_constant_and_padding(name, n, box, size):
    img, reg, st = _case(n, box, size)
    x0, y0, x1, y1 = reg
    assert np.array_equal(R.resample(img[y0:y1, x0:x1], x1 - x0, y1 - y0), img[y0:y1, x0:x1])   # its own size: its pixels
    const = np.broadcast_to(np.asarray((7, 130, 255), np.uint8), img.shape)
    assert (R.crop(const, reg, st) == (7, 130, 255)).all()                                       # a constant stays
    # "pad" writes pad_value outside the inner rectangle and the stretch rule's values inside it
    ox, oy, iw, ih = R.inner_rect("pad", x1 - x0, y1 - y0, *size)
    got, outside = R.crop(img, reg, dict(st, fit="pad")), np.ones(size[::-1], bool)
    outside[oy:oy + ih, ox:ox + iw] = False
    assert (iw == size[0] or ih == size[1]) and (got[outside] == (9, 200, 31)).all()
    assert (R.crop(const, reg, dict(st, fit="pad"))[~outside] == (7, 130, 255)).all()
    assert np.array_equal(got[oy:oy + ih, ox:ox + iw], R.crop(img, reg, dict(st, size=(iw, ih))))


def test_against_pillow():
    """Pillow's resize(size, BILINEAR, box=region): the same filter in other arithmetic (22-bit coefficients, an 8-bit
    intermediate) and, inside a larger image, over other pixels -- its outermost taps reach past the box.  Two figures,
    measured on the CPU over CASES, asserted with one LSB of margin: box=region, and the region cut out first"""
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed")
    worst_box = worst_cut = 0
    for name, n, box, size in R.CASES:
        img, reg, st = _case(n, box, size)
        got = R.crop(img, reg, st).astype(int)
        boxed = np.abs(got - np.asarray(Image.fromarray(img).resize(size, Image.BILINEAR, box=reg))).max()
        cut = np.abs(got - np.asarray(Image.fromarray(img[reg[1]:reg[3], reg[0]:reg[2]]).resize(size, Image.BILINEAR))).max()
        print(name, "box=region:", boxed, "region cut out:", cut)
        worst_box, worst_cut = max(worst_box, boxed), max(worst_cut, cut)
    assert worst_box <= PILLOW_MAX + 1 and worst_cut <= PILLOW_CUT_MAX + 1, (worst_box, worst_cut)


def test_settings_and_inferencer_argument():
    from codetr import hip_ops
    from codetr.inferencer import Inferencer, cropped_rows

    assert hip_ops.CROPS == R.DEFAULTS and hip_ops.CROP_FITS == ("stretch", "pad")
    assert hip_ops.crop_settings(dict(size=[128, 256])) == dict(R.DEFAULTS, size=(128, 256))
    t = hip_ops.crop_settings(dict(size=(8, 512), tensor=dict(mean=[1, 2, 3]), download=False))["tensor"]
    assert t == dict(mean=(1.0, 2.0, 3.0), std=(1.0, 1.0, 1.0), dtype=torch.float16)
    meta = dict(classes=["person", "face", "plate"])
    bad = dict(size=[None, (7, 8), (8, 513), (8,), (8.5, 8), "8x8"], fit=["crop", 0], expand=[-0.1, 1.5, float("nan")],
               score_thr=["0.3", None, float("nan")], pad_value=[(0, 0), (0, 0, 256), 0], max_per_img=[0, 257, 1.5, True],
               download=[0, False], radius=[3], classes=[["car"], [3], "person", []],
               tensor=[1, dict(scale=1), dict(std=(1, 0, 1)), dict(mean=(1, 2)), dict(dtype=torch.float64)])
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):     # bad settings raise at construction, naming the key
                Inferencer(None, SWIN, meta, crops={**dict(size=(16, 8)), key: v})
    with pytest.raises(ValueError, match="size"):
        Inferencer(None, SWIN, meta, crops={})
    assert Inferencer(None, SWIN, None).crops is None
    inf = Inferencer(None, SWIN, meta, crops=dict(size=(16, 8), classes=["face", 1], score_thr=0.5, max_per_img=3))
    assert inf.crops["classes"] == [1] and inf.crops["select"].tolist() == [0, 1, 0]
    nan, big = float("nan"), float("inf")
    pred = dict(labels=[1, 1, 0, 1, 1, 1, 1, 1, 1, 1], scores=[0.9, 0.5, 0.9, nan, 0.6, 0.499, 0.7, 0.7, 0.8, 0.9],
                bboxes=[[0, 0, 9, 9], [1, 1, 2, 2], [0, 0, 9, 9], [0, 0, 9, 9], [0, big, 1, 1], [0, 0, 9, 9],
                        [3.0, 0, 3.0, 9], [50, 50, 60, 60], [2, 2, 4, 4], [0, 0, 1, 1]])
    # the threshold's edge is in; other class, NaN score, infinite box, empty region (and the box outside 20 x 30) out; cut at 3
    assert cropped_rows(pred, inf.crops) == [0, 1, 7] and cropped_rows(pred, inf.crops, (20, 30)) == [0, 1, 8]


def test_host_check_of_the_argument_checks(tmp_path):
    """csrc/crops_args.h as a stand-alone program under -fsanitize=address,undefined, nothing preloaded"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "crops_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "crops_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([exe], capture_output=True, text=True) if subprocess.run(cmd + san, capture_output=True).returncode == 0 else None
    if r is not None and r.returncode != 0:
        # a finding of the program or of a sanitizer is a failure; only a runtime that cannot start in this process
        # environment (no check has printed, no sanitizer report) sends us to the plain build
        assert not any(t in r.stdout + r.stderr for t in ("FAIL", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")), \
            r.stdout[-2000:] + r.stderr[-2000:]
    if r is None or r.returncode != 0:   # no sanitizer runtimes: the same program without them still holds every answer
        subprocess.run(cmd, check=True, capture_output=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("clean"), r.stdout[-2000:] + r.stderr[-2000:]
