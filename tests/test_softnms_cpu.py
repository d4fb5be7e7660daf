"""CPU: the soft-NMS post-processing without a GPU -- hand-derived answers of the reference the GPU tests compare the
kernel with (tests/softnms_ref.py), its agreement with the literal sequential form of mmcv's algorithm, how `Inferencer`
reads the mode from the shipped configs, and the argument contract of codetr_postprocess_softnms_* (every rejection
happens on the host before any HIP call; the launch recorder proves that nothing was enqueued)."""
import ctypes
import os

import numpy as np
import pytest

import softnms_ref as R
from conftest import ROOT

F = np.float32
E_BADARG, E_TOO_LARGE = -1, -3
CONFIGS = [os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", f) for f in
           ("co_dino_5scale_r50_lsj_8xb2_1x_coco.py", "co_dino_5scale_r50_8xb2_1x_coco.py",
            "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")]
A, B09 = [0, 0, 10, 10], [0, 0, 10, 9]    # IoU 90 / 100


# ---- 1. known answers ---------------------------------------------------------------------------------------------
def test_linear_decays_the_second_box_by_one_minus_iou():
    idx, sc = R.soft_nms([A, B09], [0.9, 0.5], [3, 3], 0.8)
    assert idx.tolist() == [0, 1]
    assert sc[0] == F(0.9) and sc[1] == F(0.5) * (F(1) - F(90) / F(100))
    assert sc.dtype == np.float32


def test_different_labels_do_not_interact():
    idx, sc = R.soft_nms([A, B09], [0.9, 0.5], [3, 4], 0.8)
    assert idx.tolist() == [0, 1] and sc.tolist() == [F(0.9), F(0.5)]


def test_naive_removes_the_second_box():
    idx, sc = R.soft_nms([A, B09], [0.9, 0.5], [3, 3], 0.8, method="naive")
    assert idx.tolist() == [0] and sc.tolist() == [F(0.9)]
    # ... and below the threshold it leaves it alone
    idx, sc = R.soft_nms([A, B09], [0.9, 0.5], [3, 3], 0.95, method="naive")
    assert idx.tolist() == [0, 1] and sc.tolist() == [F(0.9), F(0.5)]


def test_iou_equal_to_the_threshold_decays():
    idx, sc = R.soft_nms([A, [0, 0, 10, 5]], [0.9, 0.5], [0, 0], 0.5)     # IoU 50 / 100 exactly
    assert idx.tolist() == [0, 1] and sc.tolist() == [F(0.9), F(0.25)]
    idx, sc = R.soft_nms([A, [0, 0, 10, 5]], [0.9, 0.5], [0, 0], float(np.nextafter(F(0.5), F(1))))
    assert sc.tolist() == [F(0.9), F(0.5)]


def test_a_box_decayed_under_min_score_disappears():
    # IoU(a, b) = IoU(b, c) = 70 / 130 >= 0.5, IoU(a, c) = 40 / 160: b falls to 0.1 * (1 - 0.538) < 0.05 and is gone,
    # so nothing is left to decay c
    a, b, c = [0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]
    idx, sc = R.soft_nms([a, b, c], [0.9, 0.1, 0.06], [1, 1, 1], 0.5, min_score=0.05)
    assert idx.tolist() == [0, 2] and sc.tolist() == [F(0.9), F(0.06)]
    # a b that survives its decay (0.2 -> 0.092) is picked second and decays c in turn
    w = F(1) - F(70) / F(130)
    idx, sc = R.soft_nms([a, b, c], [0.9, 0.2, 0.06], [1, 1, 1], 0.5, min_score=0.01)
    assert idx.tolist() == [0, 1, 2] and sc.tolist() == [F(0.9), F(0.2) * w, F(0.06) * w]
    idx, sc = R.soft_nms([a, b, c], [0.9, 0.2, 0.06], [1, 1, 1], 0.5, min_score=0.05)   # ... under min_score: c is gone
    assert idx.tolist() == [0, 1] and sc.tolist() == [F(0.9), F(0.2) * w]


def test_the_global_maximum_is_emitted_even_below_min_score():
    idx, sc = R.soft_nms([A, [20, 20, 30, 30], [40, 40, 50, 50]], [0.0002, 0.0005, 0.0005], [0, 1, 2], 0.8)
    assert idx.tolist() == [1] and sc.tolist() == [F(0.0005)]      # ties: the lowest index is the maximum


def test_zero_area_pair_has_nan_overlap_and_weight_one():
    z = [5, 5, 5, 5]
    for method in ("linear", "naive"):
        idx, sc = R.soft_nms([z, z], [0.9, 0.5], [0, 0], 0.3, method=method)
        assert idx.tolist() == [0, 1] and sc.tolist() == [F(0.9), F(0.5)]


def test_max_keep_cuts_after_the_sort_by_decayed_score():
    boxes, scores, labels = [A, B09, [40, 40, 50, 50]], [0.9, 0.8, 0.5], [0, 0, 1]
    idx, sc = R.soft_nms(boxes, scores, labels, 0.8)
    assert idx.tolist() == [0, 2, 1]                                # 0.8 decayed to 0.08 sorts behind 0.5
    idx, sc = R.soft_nms(boxes, scores, labels, 0.8, max_keep=2)
    assert idx.tolist() == [0, 2] and sc.tolist() == [F(0.9), F(0.5)]


def test_ties_go_to_the_lowest_index_and_the_threshold_is_strict():
    idx, sc = R.soft_nms([A, A, A], [0.5, 0.5, 0.7], [0, 0, 1], 0.8, score_threshold=F(0.5))
    assert idx.tolist() == [2]
    idx, sc = R.soft_nms([A, [20, 20, 30, 30], [40, 40, 50, 50]], [0.5, 0.5, -0.0], [0, 0, 0], 0.8, min_score=-1.0)
    assert idx.tolist() == [0, 1, 2]
    idx, sc = R.soft_nms([A, A], [float("nan"), 0.5], [0, 0], 0.8, score_threshold=F(0.1))   # NaN fails the threshold
    assert idx.tolist() == [1]


# ---- 2. the per-label form equals the literal sequential form -------------------------------------------------------
def _case(rng, n, classes, clustered):
    if clustered:
        centres = rng.uniform(20, 200, (max(1, n // 8), 2))
        c = centres[rng.integers(0, len(centres), n)] + rng.uniform(-4, 4, (n, 2))
        wh = 60 + rng.uniform(-5, 5, (n, 2))
    else:
        c, wh = rng.uniform(0, 800, (n, 2)), rng.uniform(2, 150, (n, 2))
    boxes = np.concatenate((c - wh / 2, c + wh / 2), 1).astype(F)
    scores = rng.permutation(np.linspace(0.0005, 0.999, n)).astype(F)      # distinct
    return boxes, scores, rng.integers(0, classes, n)


def test_per_label_form_equals_the_literal_sequential_form():
    rng = np.random.default_rng(2024)
    dropped = 0
    for trial in range(160):
        n = int(rng.integers(1, 60))
        boxes, scores, labels = _case(rng, n, (1, 3, 80)[trial % 3], trial % 2 == 0)
        for method in ("linear", "naive"):
            thr, mn = (0.3, 0.8)[(trial // 2) % 2], (1e-3, 0.05)[(trial // 4) % 2]
            idx, sc = R.soft_nms(boxes, scores, labels, thr, method, mn)
            if len(set(sc.tolist())) != len(sc):
                continue                                            # (a tie after decay: the forms may order it differently)
            lidx, lsc = R.soft_nms_literal(boxes, scores, labels, thr, method, mn)
            assert idx.tolist() == lidx.tolist(), (trial, method)
            assert sc.tobytes() == lsc.tobytes(), (trial, method)
            dropped += len(idx) < n
    assert dropped > 100


# ---- 3. Inferencer reads the mode from the config -------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS)
def test_nms_settings_of_the_shipped_configs(cfg):
    from codetr.config import Config
    from codetr.inferencer import Inferencer, nms_settings

    test_cfg = Config.fromfile(cfg).model.test_cfg[0]
    s = nms_settings(test_cfg)
    assert (s["type"], s["max_per_img"]) == ("nms", None)
    s = nms_settings(test_cfg, "config")
    assert (s["type"], s["method"], s["min_score"], s["max_per_img"]) == ("soft_nms", "linear", 1e-3, 300)
    assert test_cfg["nms"]["iou_threshold"] == 0.8
    assert nms_settings(test_cfg, "nms")["type"] == "nms" and nms_settings(test_cfg, "nms")["max_per_img"] == 300
    with pytest.raises(ValueError, match="softnms"):
        nms_settings(test_cfg, "softnms")
    if cfg == CONFIGS[0]:
        return    # (the LSJ base config carries no test pipeline: an Inferencer is built from its two children)
    inf = Inferencer(None, cfg, None)
    assert inf.with_nms and inf.nms_type == "nms" and not inf.soft and inf.max_per_img is None and inf.iou_threshold == 0.8
    inf = Inferencer(None, cfg, None, nms_type="config")
    assert inf.with_nms and inf.soft and inf.nms_type == "soft_nms"
    assert (inf.iou_threshold, inf.soft_method, inf.min_score, inf.max_per_img) == (0.8, "linear", 1e-3, 300)
    inf = Inferencer(None, cfg, None, nms_type="nms", iou_threshold=0.5)
    assert inf.with_nms and not inf.soft and inf.max_per_img == 300 and inf.iou_threshold == 0.5
    inf = Inferencer(None, cfg, None, nms_type="soft_nms")
    assert inf.soft and inf.max_per_img == 300
    with pytest.raises(ValueError, match="softnms"):
        Inferencer(None, cfg, None, nms_type="softnms")


def test_inferencer_rejects_the_gaussian_method(tmp_path):
    from codetr.inferencer import Inferencer

    base, child = open(CONFIGS[0]).read(), open(CONFIGS[1]).read()
    entry = "nms=dict(type='soft_nms', iou_threshold=0.8)"
    assert entry in base

    def config(nms):
        d = tmp_path / nms.split("'")[1]
        d.mkdir()
        (d / os.path.basename(CONFIGS[0])).write_text(base.replace(entry, f"nms=dict(type='soft_nms', {nms})"))
        (d / os.path.basename(CONFIGS[1])).write_text(child)     # inherits from the file next to it
        return str(d / os.path.basename(CONFIGS[1]))

    for method, exc in (("gaussian", NotImplementedError), ("quadratic", ValueError)):
        path = config(f"method='{method}', iou_threshold=0.8")
        assert Inferencer(None, path, None).nms_type == "nms"          # the default never looks at it
        with pytest.raises(exc, match=method):
            Inferencer(None, path, None, nms_type="config")
    inf = Inferencer(None, config("method='naive', iou_threshold=0.6, min_score=0.01"), None, nms_type="config")
    assert (inf.iou_threshold, inf.soft_method, inf.min_score, inf.soft) == (0.6, "naive", 0.01, True)


# ---- 4. C ABI argument contract -------------------------------------------------------------------------------------
@pytest.fixture
def lib():
    from codetr import _cabi

    _cabi.RECORDER = []
    try:
        yield _cabi.load()
        assert _cabi.RECORDER == []   # no rejected call reached a launch
    finally:
        _cabi.RECORDER = None


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_postprocess_softnms_rejects_bad_arguments(lib, suffix):
    from codetr import _cabi

    assert _cabi.ABI_VERSION == 54 and "postprocess_softnms" in _cabi.CALLS
    assert _cabi.SOFTNMS_METHODS == {"naive": 0, "linear": 1}
    f = getattr(lib, "codetr_postprocess_softnms_" + suffix)
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first

    def call(ptrs=(one,) * 9, N=2, Q=300, method=1, iou=0.8, min_score=1e-3):
        b, s, l, d, bo, so, lo, io, c = ptrs
        return f(None, b, s, l, d, N, Q, 1, 0.3, method, iou, min_score, 300, bo, so, lo, io, c)

    for i in range(9):
        ptrs = [one] * 9
        ptrs[i] = None
        assert call(ptrs) == E_BADARG, i
    assert call(N=0) == E_BADARG
    assert call(Q=0) == E_BADARG
    assert call(Q=-5) == E_BADARG
    assert call(method=2) == E_BADARG
    assert call(method=-1) == E_BADARG
    for v in (float("nan"), float("inf"), -float("inf")):
        assert call(iou=v) == E_BADARG
        assert call(min_score=v) == E_BADARG
    assert call(Q=1025) == E_TOO_LARGE
    assert call(Q=1025, method=0) == E_TOO_LARGE
