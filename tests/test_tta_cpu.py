"""CPU: test-time augmentation -- known answers of the merge reference (tests/tta_ref.py), how `Inferencer(tta=...)`
reads its argument (codetr.inferencer.tta_settings), and the argument contract of codetr_preprocess_views_u8_* and
codetr_tta_merge_* (include/codetr_hip.h), whose rejections happen on the host before any HIP call."""
import ctypes
import glob
import os

import numpy as np
import pytest

import tta_ref as R
from conftest import ROOT

E_BADARG, E_TOO_LARGE = -1, -3
F = np.float32
CONFIGS = sorted(glob.glob(os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_*.py")))


# ---- 1. the reference ---------------------------------------------------------------------------------------------
def _two_views_of_one_box():
    """a 100-wide image; view 0 sees the box (10, 20, 40, 60), the flipped view 1 sees its mirror (60, 20, 90, 60)"""
    boxes = np.array([[[10, 20, 40, 60]], [[60, 20, 90, 60]]], F)
    scores = np.array([[0.9], [0.8]], F)
    labels = np.array([[3], [3]])
    return boxes, scores, labels, np.array([1, 1]), [False, True], 100.0


def test_two_views_of_one_box_collapse_under_hard_nms():
    c, sc, bx = R.merge(*_two_views_of_one_box(), mode="nms", iou_threshold=0.5)
    assert c.tolist() == [0] and sc.tolist() == [F(0.9)] and bx.tolist() == [[10, 20, 40, 60]]
    # without the un-flip the two boxes do not overlap and both stay
    b, s, l, cnt, _, w = _two_views_of_one_box()
    assert R.merge(b, s, l, cnt, [False, False], w, mode="nms", iou_threshold=0.5)[0].tolist() == [0, 1]


def test_two_views_of_one_box_decay_under_linear_soft_nms():
    c, sc, bx = R.merge(*_two_views_of_one_box(), mode="linear", iou_threshold=0.3, min_score=1e-3)
    assert c.tolist() == [0]                       # IoU 1: 0.8 * (1 - 1) = 0 < min_score, the second view leaves
    b, s, l, cnt, fl, w = _two_views_of_one_box()
    b[1, 0] = [60, 20, 100, 60]                    # un-flipped (0, 20, 40, 60): IoU with (10, 20, 40, 60) = 30 / 40
    c, sc, bx = R.merge(b, s, l, cnt, fl, w, mode="linear", iou_threshold=0.3)
    assert c.tolist() == [0, 1] and bx[1].tolist() == [0, 20, 40, 60]
    assert sc[0] == F(0.9) and sc[1] == F(F(0.8) * (F(1) - F(1200) / (F(1200) + F(1600) - F(1200))))
    c, sc, _ = R.merge(b, s, l, cnt, fl, w, mode="naive", iou_threshold=0.3)
    assert c.tolist() == [0]


def test_reference_rules():
    # the hard rule is IoU > threshold: an IoU equal to it keeps both
    boxes = np.array([[[0, 0, 2, 2], [0, 0, 2, 1]]], F)           # IoU 2 / 4 = 0.5
    scores = np.array([[0.5, 0.5]], F)
    labels = np.array([[1, 1]])
    assert R.merge(boxes, scores, labels, [2], [False], 10.0, "nms", 0.5)[0].tolist() == [0, 1]
    assert R.merge(boxes, scores, labels, [2], [False], 10.0, "nms", 0.49)[0].tolist() == [0]   # the tie: lowest c wins
    # different labels never interact; count cuts a view's rows; the order is by score, ties by ascending c
    labels2 = np.array([[1, 2]])
    assert R.merge(boxes, scores, labels2, [2], [False], 10.0, "nms", 0.1)[0].tolist() == [0, 1]
    assert R.merge(boxes, scores, labels, [1], [False], 10.0, "nms", 0.1)[0].tolist() == [0]
    assert R.merge(boxes, scores, labels, [0], [False], 10.0, "nms", 0.1)[0].tolist() == []
    b3 = np.array([[[0, 0, 1, 1]], [[5, 5, 6, 6]], [[8, 8, 9, 9]]], F)
    s3 = np.array([[0.2], [0.7], [0.7]], F)
    l3 = np.array([[0], [0], [0]])
    c, sc, _ = R.merge(b3, s3, l3, [1, 1, 1], [False] * 3, 10.0, "nms", 0.5)
    assert c.tolist() == [1, 2, 0]
    assert R.merge(b3, s3, l3, [1, 1, 1], [False] * 3, 10.0, "nms", 0.5, max_keep=2)[0].tolist() == [1, 2]
    # un-flip: one fp32 subtraction per coordinate
    u = R.unflip(np.array([[0.1, 1, 0.7, 2]], F), 3.3)
    assert u[0, 0] == F(3.3) - F(0.7) and u[0, 2] == F(3.3) - F(0.1) and u[0, 1] == 1 and u[0, 3] == 2


# ---- 2. tta_settings ----------------------------------------------------------------------------------------------
def test_tta_settings_on_dicts():
    from codetr.inferencer import tta_settings

    assert tta_settings(None, None) is None
    t = tta_settings(None, dict(scales=[(1333, 800), (2000, 1200)], flip=True, nms=dict(type="nms", iou_threshold=0.6),
                                max_per_img=100))
    assert t["scales"] == [(1333, 800), (2000, 1200)] and t["flip"] is True and t["max_per_img"] == 100
    assert t["nms"] == dict(type="nms", iou_threshold=0.6, method="linear", min_score=1e-3)
    # the view order: v = s * 2 + f, unflipped first
    assert t["views"] == [((1333, 800), False), ((1333, 800), True), ((2000, 1200), False), ((2000, 1200), True)]
    t = tta_settings(None, dict(scales=[(640, 480)], nms=dict(type="soft_nms", iou_threshold=0.4, method="naive")))
    assert t["flip"] is False and t["views"] == [((640, 480), False)] and t["max_per_img"] is None
    assert t["nms"] == dict(type="soft_nms", iou_threshold=0.4, method="naive", min_score=1e-3)
    assert tta_settings(None, dict(scales=(640, 480)))["scales"] == [(640, 480)]
    with pytest.raises(NotImplementedError):
        tta_settings(None, dict(scales=[(640, 480)], nms=dict(type="soft_nms", method="gaussian")))
    with pytest.raises(ValueError):
        tta_settings(None, dict(scales=[(640, 480)], nms=dict(type="soft_nms", method="cubic")))
    with pytest.raises(NotImplementedError):
        tta_settings(None, dict(scales=[(640, 480)], nms=dict(type="wbf")))
    with pytest.raises(ValueError):
        tta_settings(None, dict(scales=[]))
    with pytest.raises(ValueError):
        tta_settings(None, dict(flip=True))
    with pytest.raises(ValueError):
        tta_settings(None, dict(scales=[(640, 480)], vflip=True))
    with pytest.raises(ValueError):
        tta_settings(None, "auto")
    assert len(tta_settings(None, dict(scales=[(100 + i, 50) for i in range(8)], flip=True))["views"]) == 16
    with pytest.raises(ValueError, match="16"):
        tta_settings(None, dict(scales=[(100 + i, 50) for i in range(9)], flip=True))


_TTA_CONFIG = """
tta_model = dict(type='DetTTAModel', tta_cfg=dict(nms=dict(type='{nms}', iou_threshold=0.6), max_per_img=100))
img_scales = [(1333, 800), (666, 400), (2000, 1200)]
tta_pipeline = [
    dict(type='LoadImageFromFile', backend_args=None),
    dict(type='TestTimeAug', transforms=[
        [dict(type='Resize', scale=s, keep_ratio=True) for s in img_scales],
        [dict(type='RandomFlip', prob=1.), dict(type='RandomFlip', prob=0.)],
        [dict(type='LoadAnnotations', with_bbox=True)],
        [dict(type='PackDetInputs', meta_keys=('img_id', 'flip'))]])]
"""


def test_tta_settings_on_an_mmdet_style_config(tmp_path):
    from codetr.config import Config
    from codetr.inferencer import tta_settings

    path = tmp_path / "tta.py"
    path.write_text(_TTA_CONFIG.format(nms="nms"))
    t = tta_settings(Config.fromfile(str(path)), "config")
    assert t["scales"] == [(1333, 800), (666, 400), (2000, 1200)] and t["flip"] is True and t["max_per_img"] == 100
    assert t["nms"]["type"] == "nms" and t["nms"]["iou_threshold"] == 0.6 and len(t["views"]) == 6
    assert t["views"][:2] == [((1333, 800), False), ((1333, 800), True)]
    path.write_text(_TTA_CONFIG.format(nms="soft_nms").replace("dict(type='RandomFlip', prob=1.), ", ""))
    t = tta_settings(Config.fromfile(str(path)), "config")
    assert t["flip"] is False and t["nms"]["type"] == "soft_nms" and t["nms"]["method"] == "linear" and len(t["views"]) == 3
    path.write_text("tta_model = dict(type='DetTTAModel', tta_cfg=dict(max_per_img=100))\n")
    with pytest.raises(ValueError):
        tta_settings(Config.fromfile(str(path)), "config")     # no tta_pipeline


@pytest.mark.parametrize("cfg", CONFIGS, ids=os.path.basename)
def test_shipped_configs_have_no_tta_entry(cfg):
    from codetr.config import Config
    from codetr.inferencer import tta_settings

    assert len(CONFIGS) == 3
    assert tta_settings(Config.fromfile(cfg), None) is None
    with pytest.raises(ValueError, match="tta_model"):
        tta_settings(Config.fromfile(cfg), "config")


def test_inferencer_constructor_takes_tta():
    from codetr.inferencer import Inferencer

    cfg = [c for c in CONFIGS if "swin_l" in c][0]
    assert Inferencer(None, cfg, dataset_meta=None).tta is None          # the default: nothing changes
    with pytest.raises(ValueError, match="tta_model"):
        Inferencer(None, cfg, dataset_meta=None, tta="config")
    inf = Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(320, 200)], flip=True))
    assert inf.tta["nms"] == dict(type="nms", iou_threshold=0.5, method="linear", min_score=1e-3)
    assert inf.tta["views"] == [((320, 200), False), ((320, 200), True)]


# ---- 3. the C entry points' argument contract ---------------------------------------------------------------------
@pytest.fixture
def lib():
    from codetr import _cabi

    _cabi.RECORDER = []
    try:
        yield _cabi.load()
        assert _cabi.RECORDER == []   # no rejected call reached a launch
    finally:
        _cabi.RECORDER = None


def test_abi_number_and_constants(lib):
    from codetr import _cabi

    assert _cabi.ABI_VERSION == 54 and lib.codetr_hip_abi_version() == 54
    assert _cabi.TTA_MAX_VIEWS == 16 and _cabi.TTA_MAX_CANDIDATES == 4096
    assert "preprocess_views" in _cabi.CALLS and "tta_merge" in _cabi.CALLS


def _table(rows):
    return (ctypes.c_int64 * (8 * len(rows)))(*[v for r in rows for v in r])


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_preprocess_views_rejects_bad_arguments(lib, suffix):
    f = getattr(lib, "codetr_preprocess_views_u8_" + suffix)
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)
    pad = (ctypes.c_int * 3)(0, 0, 0)
    row = (0, 10, 20, 5, 10, 8, 16, 1)
    ok = dict(src=one, nbytes=600, N=1, tab=_table([row]), H=8, W=16, mean=mean, std=std, pad=pad, dst=one)

    def call(**kw):
        a = dict(ok, **kw)
        return f(None, a["src"], a["nbytes"], a["N"], a["tab"], a["H"], a["W"], a["mean"], a["std"], a["pad"], 0.0,
                 a["dst"], None)

    for name in ("src", "dst", "tab", "mean", "std", "pad"):
        assert call(**{name: None}) == E_BADARG, name
    assert call(tab=_table([row[:7] + (2,)])) == E_BADARG            # flip is 0 or 1
    assert call(tab=_table([row[:7] + (-1,)])) == E_BADARG
    assert call(N=2, tab=_table([row[:7] + (0,), row[:7] + (2,)])) == E_BADARG
    # everything else as the batch entry
    assert call(N=0) == E_BADARG
    assert call(H=0) == E_BADARG
    assert call(N=33, tab=_table([row] * 33)) == E_TOO_LARGE
    assert call(H=65536) == E_TOO_LARGE
    assert call(std=(ctypes.c_float * 3)(1, 0, 1)) == E_BADARG
    assert call(pad=(ctypes.c_int * 3)(0, 256, 0)) == E_BADARG
    assert call(H=7) == E_BADARG
    assert call(tab=_table([(0, 10, 20, 9, 10, 8, 16, 0)])) == E_BADARG
    assert call(nbytes=599) == E_BADARG
    assert call(tab=_table([(-1, 10, 20, 5, 10, 8, 16, 0)])) == E_BADARG
    assert call(tab=_table([(0, 40000, 1, 5, 10, 8, 16, 1)]), nbytes=120000) == E_TOO_LARGE


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_tta_merge_rejects_bad_arguments(lib, suffix):
    f = getattr(lib, "codetr_tta_merge_" + suffix)
    one = ctypes.c_void_p(16)

    def call(ptrs=None, V=2, N=3, Q=300, flip=0b10, mode=0, iou=0.5, min_score=1e-3, keep=100):
        b, s, l, c, w, bo, so, lo, io, co = ptrs or [one] * 10
        return f(None, b, s, l, c, V, N, Q, flip, w, mode, iou, min_score, keep, bo, so, lo, io, co)

    for i in range(10):
        ptrs = [one] * 10
        ptrs[i] = None
        assert call(ptrs) == E_BADARG, i
    assert call(V=0) == E_BADARG
    assert call(N=0) == E_BADARG
    assert call(Q=0) == E_BADARG
    assert call(Q=-5) == E_BADARG
    assert call(flip=0b100) == E_BADARG                              # a flip bit at or above V
    assert call(V=1, Q=10, flip=0b10) == E_BADARG
    assert call(mode=3) == E_BADARG
    assert call(mode=-1) == E_BADARG
    assert call(iou=float("nan")) == E_BADARG
    assert call(iou=float("inf")) == E_BADARG
    assert call(mode=2, min_score=float("nan")) == E_BADARG
    assert call(V=17, Q=1, flip=0) == E_TOO_LARGE                    # CODETR_TTA_MAX_VIEWS
    assert call(V=1, Q=4097, flip=0) == E_TOO_LARGE                  # V * Q = 4097
    assert call(V=7, Q=586, flip=0) == E_TOO_LARGE                   # 4102
    assert call(V=16, Q=257, flip=0) == E_TOO_LARGE
