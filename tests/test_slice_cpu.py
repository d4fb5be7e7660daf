"""CPU: sliced inference -- the tile grid by hand, how `Inferencer(slicing=...)` reads its argument, its limits, known
answers of the merge reference (tests/slice_ref.py), and the argument contract of codetr_preprocess_tiles_u8_* and
codetr_slice_merge_* (include/codetr_hip.h), whose rejections happen on the host before any HIP call."""
import ctypes
import glob
import os

import numpy as np
import pytest

import slice_ref as R
from conftest import ROOT

E_BADARG, E_TOO_LARGE = -1, -3
F = np.float32
SWIN = [c for c in sorted(glob.glob(os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_*.py"))) if "swin_l" in c][0]


def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    return Inferencer(None, SWIN, dataset_meta=None, **kw)


# ---- 1. the tile grid ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,starts,length", [(1000, [0, 410, 488], 512), (700, [0, 188], 512), (512, [0], 512),
                                             (513, [0, 1], 512), (300, [0], 300)])
def test_grid_axis_known_answers(L, starts, length):
    """t = 512, o = 0.2: the step is 512 - int(102.4) = 410; by hand"""
    from codetr.inferencer import Inferencer

    along_x = Inferencer.slice_grid(7, L, (512, 512), 0.2)
    assert along_x == [(0, x, 7, length) for x in starts]
    along_y = Inferencer.slice_grid(L, 7, (512, 512), (0.5, 0.2))
    assert along_y == [(y, 0, length, 7) for y in starts]
    assert R.axis_starts(L, 512, 0.2) == (starts, length)


def test_grid_is_y_major():
    from codetr.inferencer import Inferencer

    tiles = Inferencer.slice_grid(700, 1000, (512, 512), 0.2)
    assert tiles == [(0, 0, 512, 512), (0, 410, 512, 512), (0, 488, 512, 512),
                     (188, 0, 512, 512), (188, 410, 512, 512), (188, 488, 512, 512)]
    assert tiles == R.grid(700, 1000, (512, 512), (0.2, 0.2))
    # a rectangular tile and an overlap per axis: steps 300 - 0 and 200 - 100
    assert Inferencer.slice_grid(450, 700, (300, 200), (0.0, 0.5)) == [
        (y, x, 200, 300) for y in (0, 100, 200, 250) for x in (0, 300, 400)]
    for H, W, tile, ov in [(1, 1, (5, 5), (0.9, 0.9)), (2160, 3840, (1280, 1280), (0.2, 0.2)), (97, 33, (10, 7), (0.95, 0.3))]:
        tiles = Inferencer.slice_grid(H, W, tile, ov)
        assert tiles == R.grid(H, W, tile, ov)
        covered = np.zeros((H, W), bool)
        for y, x, h, w in tiles:
            assert 0 <= y and y + h <= H and 0 <= x and x + w <= W and h == min(tile[1], H) and w == min(tile[0], W)
            covered[y:y + h, x:x + w] = True
        assert covered.all() and len(set(tiles)) == len(tiles)
    with pytest.raises(ValueError):
        Inferencer.slice_grid(10, 10, (5, 5), 1.0)


# ---- 2. settings and limits ---------------------------------------------------------------------------------------
def test_slicing_settings_and_defaults():
    from codetr.inferencer import slicing_settings

    assert slicing_settings(None) is None and _inferencer().slicing is None
    s = slicing_settings(dict(tile=(640, 480)))
    assert s == dict(tile=(640, 480), overlap=(0.2, 0.2), full_image=True,
                     merge=dict(type="nmm", metric="ios", threshold=0.5, class_agnostic=False), max_per_img=300,
                     tile_batch=8)
    s = _inferencer(slicing=dict(tile=[512, 512], overlap=(0.1, 0.3), full_image=False, max_per_img=None, tile_batch=3,
                                 merge=dict(type="nms", metric="iou", threshold=0.6, class_agnostic=True))).slicing
    assert s == dict(tile=(512, 512), overlap=(0.1, 0.3), full_image=False,
                     merge=dict(type="nms", metric="iou", threshold=0.6, class_agnostic=True), max_per_img=None,
                     tile_batch=3)
    for bad in (dict(), dict(tile=(0, 5)), dict(tile=(5,)), dict(tile=(5, 5), overlap=1.0), dict(tile=(5, 5), overlap=-0.1),
                dict(tile=(5, 5), tile_batch=0), dict(tile=(5, 5), tiles=3), "config",
                dict(tile=(5, 5), merge=dict(threshold=float("nan"))), dict(tile=(5, 5), merge=dict(iou=0.5))):
        with pytest.raises(ValueError):
            slicing_settings(bad)


def test_unknown_metric_or_mode():
    from codetr.inferencer import slicing_settings

    with pytest.raises(ValueError, match="metric"):
        slicing_settings(dict(tile=(5, 5), merge=dict(metric="giou")))
    with pytest.raises(ValueError, match="type"):
        slicing_settings(dict(tile=(5, 5), merge=dict(type="soft_nms")))
    with pytest.raises(ValueError, match="type"):
        _inferencer(slicing=dict(tile=(5, 5), merge=dict(type="greedy")))


def test_slicing_with_tta_is_not_built():
    with pytest.raises(NotImplementedError, match="tta"):
        _inferencer(slicing=dict(tile=(512, 512)), tta=dict(scales=[(320, 200)]))


def test_view_and_candidate_limits():
    """64 views: raised from the row table, before anything is uploaded or launched (so it runs without a GPU);
    4096 candidates: the check the chunk makes once the first forward has told it Q"""
    from codetr import hip_ops

    assert hip_ops.SLICE_MAX_VIEWS == 64
    inf = _inferencer(slicing=dict(tile=(100, 100), overlap=0.0))
    rows, metas, table, _ = inf.slice_rows([0], [(700, 900)])                  # 7 x 9 tiles + the image = 64 views
    assert len(rows) == 64 and table == [list(range(64))]
    with pytest.raises(ValueError, match="64"):
        inf.slice_rows([0], [(701, 900)])                                      # 8 x 9 + 1
    with pytest.raises(ValueError, match="64"):
        inf([np.zeros((701, 900, 3), np.uint8)], device="cuda:0", batch_size=2)
    inf.slice_limits(13, 300)
    inf.slice_limits(64, 64)
    with pytest.raises(ValueError, match="4096"):
        inf.slice_limits(14, 300)                                              # (T + 1) * Q = 4200
    with pytest.raises(ValueError, match="4096"):
        inf.slice_limits(5, 900)


def test_slice_rows_known_answers():
    """a 600x1000 and a 300x400 image, 512-tiles at overlap 0.2, scale (2048, 1280): the first has
    2 x 3 tiles + itself, the second is smaller than a tile: one 300x400 tile + itself; absent views are -1"""
    inf = _inferencer(slicing=dict(tile=(512, 512)))
    inf.scale, inf.pad_size_divisor = (2048, 1280), 32
    rows, metas, table, hw = inf.slice_rows([0, 1800000], [(600, 1000), (300, 400)])
    assert table == [[0, 1, 2, 3, 4, 5, 6], [7, 8, -1, -1, -1, -1, -1]]
    assert [r[:7] for r in rows] == [(0, 600, 1000, y, x, 512, 512) for y in (0, 88) for x in (0, 410, 488)] + [
        (0, 600, 1000, 0, 0, 600, 1000), (1800000, 300, 400, 0, 0, 300, 400), (1800000, 300, 400, 0, 0, 300, 400)]
    # 512x512 into (2048, 1280): factor min(2048/512, 1280/512) = 2.5 -> 1280x1280; 600x1000: min(2.048, 2.1333) -> 1229x2048
    assert rows[0][7:] == (1280, 1280, 1280, 1280) and rows[6][7:] == (1229, 2048, 1229, 2048)
    assert rows[7][7:] == (1280, 1707, 1280, 1707)
    assert hw == (1280, 2048) and metas[6]["pad_shape"] == (1248, 2048) and metas[7]["pad_shape"] == (1280, 1728)
    assert [m["origin"] for m in metas[:7]] == [(0, 0), (410, 0), (488, 0), (0, 88), (410, 88), (488, 88), (0, 0)]
    assert metas[0]["scale_factor"] == (2.5, 2.5) and metas[6]["scale_factor"] == (2048 / 1000, 1229 / 600)


# ---- 3. the merge reference, three boxes by hand -------------------------------------------------------------------
def _one(boxes, scores, labels=(1, 1, 1), origin=(0, 0), size=(100, 100), **kw):
    b = np.asarray(boxes, F)[None]
    n = b.shape[1]
    return R.merge(b, np.asarray(scores, F)[None], np.asarray(labels)[None, :n], [n], [0], [origin], size, **kw)


def test_ios_above_the_threshold_while_iou_is_below():
    """a 10x10 box inside a 40x40 one: inter 100, IoU 100 / 1600 = 0.0625, IoS 100 / 100 = 1; a far box stays"""
    boxes = [[0, 0, 40, 40], [10, 10, 20, 20], [60, 60, 80, 80]]
    c, sc, bx, _ = _one(boxes, [0.9, 0.8, 0.7], metric="iou", mode="nms", threshold=0.5)
    assert c.tolist() == [0, 1, 2]
    c, sc, bx, _ = _one(boxes, [0.9, 0.8, 0.7], metric="ios", mode="nms", threshold=0.5)
    assert c.tolist() == [0, 2] and bx.tolist() == [[0, 0, 40, 40], [60, 60, 80, 80]]
    # another label is never matched, unless class_agnostic
    c, _, _, lab = _one(boxes, [0.9, 0.8, 0.7], labels=(1, 2, 1), metric="ios", mode="nms")
    assert c.tolist() == [0, 1, 2] and lab.tolist() == [1, 2, 1]
    c, _, _, lab = _one(boxes, [0.9, 0.8, 0.7], labels=(1, 2, 1), metric="ios", mode="nms", class_agnostic=True)
    assert c.tolist() == [0, 2] and lab.tolist() == [1, 1]


def test_nmm_union_is_against_the_picks_own_box():
    """k = (10, 10, 30, 30) absorbs (20, 5, 35, 25) (inter 10 x 15 = 150, IoS 150 / 300 = 0.5 -> at 0.4 a hit): the union
    is (10, 5, 35, 30).  The third box (32, 0, 50, 10) overlaps the union but not k: it stays, with k's score first"""
    boxes = [[10, 10, 30, 30], [20, 5, 35, 25], [32, 0, 50, 10]]
    c, sc, bx, lab = _one(boxes, [0.9, 0.8, 0.7], labels=(4, 4, 4), metric="ios", mode="nmm", threshold=0.4)
    assert c.tolist() == [0, 2] and sc.tolist() == [F(0.9), F(0.7)] and lab.tolist() == [4, 4]
    assert bx.tolist() == [[10, 5, 35, 30], [32, 0, 50, 10]]
    # exactly at the threshold nothing is absorbed ('>' is strict)
    c, _, bx, _ = _one(boxes, [0.9, 0.8, 0.7], metric="ios", mode="nmm", threshold=0.5)
    assert c.tolist() == [0, 1, 2] and bx.tolist() == boxes
    # the lower score is the absorbed one whatever the order in memory; ties go to the lowest c
    c, sc, bx, _ = _one(boxes, [0.8, 0.9, 0.7], metric="ios", mode="nmm", threshold=0.4)
    assert c.tolist() == [1, 2] and bx[0].tolist() == [10, 5, 35, 30]
    c, _, _, _ = _one(boxes, [0.8, 0.8, 0.8], metric="ios", mode="nmm", threshold=0.4)
    assert c.tolist() == [0, 2]


def test_origin_shift_clip_and_zero_area():
    """a tile at (90, 95) of a 100x100 image: (-5, -5, 5, 3) -> (85, 90, 95, 98); (20, 20, 30, 30) -> (110, 115, 120, 125)
    clips to (100, 100, 100, 100), a box of no area that matches nothing (0 / 0 compares false) -- not even its twin"""
    boxes = [[-5, -5, 5, 3], [20, 20, 30, 30], [20, 20, 30, 30]]
    for metric in ("iou", "ios"):
        for mode in ("nms", "nmm"):
            c, sc, bx, _ = _one(boxes, [0.9, 0.8, 0.7], origin=(90, 95), metric=metric, mode=mode, threshold=0.0)
            assert c.tolist() == [0, 1, 2]
            assert bx.tolist() == [[85, 90, 95, 98], [100, 100, 100, 100], [100, 100, 100, 100]]
    c, _, bx, _ = _one([[float("nan"), -3, 7, 200]], [0.5], origin=(1, 2))
    assert bx.tolist() == [[0, 0, 8, 100]]                                       # NaN -> 0, the rest clipped
    # absent views, zero counts, max_keep
    b = np.zeros((2, 3, 4), F)
    b[:, :, 2:] = 10
    b[1, :, 0] = 50
    b[1, :, 2] = 60
    s = np.asarray([[0.5, 0.4, 0.3], [0.6, 0.2, 0.1]], F)
    lab = np.zeros((2, 3), np.int64)
    c, sc, _, _ = R.merge(b, s, lab, [3, 1], [-1, 1, 2, 0], np.zeros((2, 2), F), (100, 100), mode="nms")
    assert c.tolist() == [3, 9] and sc.tolist() == [F(0.6), F(0.5)]             # c = v * Q + j: views 1 and 3
    c, _, _, _ = R.merge(b, s, lab, [3, 1], [-1, 1, 2, 0], np.zeros((2, 2), F), (100, 100), mode="nms", max_keep=1)
    assert c.tolist() == [3]
    assert len(R.merge(b, s, lab, [0, 0], [0, 1], np.zeros((2, 2), F), (100, 100))[0]) == 0


# ---- 4. the C entry points' argument contract ---------------------------------------------------------------------
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
    from codetr import _cabi, hip_ops

    assert _cabi.ABI_VERSION == 54 and lib.codetr_hip_abi_version() == 54
    assert _cabi.SLICE_MAX_VIEWS == hip_ops.SLICE_MAX_VIEWS == 64
    assert "preprocess_tiles" in _cabi.CALLS and "slice_merge" in _cabi.CALLS
    assert _cabi.SLICE_METRICS == dict(iou=0, ios=1) and _cabi.SLICE_MODES == dict(nms=0, nmm=1)
    header = open(os.path.join(ROOT, "include", "codetr_hip.h")).read()
    for line in ("#define CODETR_SLICE_MAX_VIEWS 64", "#define CODETR_SLICE_IOU 0", "#define CODETR_SLICE_IOS 1",
                 "#define CODETR_SLICE_NMS 0", "#define CODETR_SLICE_NMM 1"):
        assert line in header


def _table(rows):
    return (ctypes.c_int64 * (11 * len(rows)))(*[v for r in rows for v in r])


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_preprocess_tiles_rejects_bad_arguments(lib, suffix):
    f = getattr(lib, "codetr_preprocess_tiles_u8_" + suffix)
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)
    pad = (ctypes.c_int * 3)(0, 0, 0)
    row = (0, 10, 20, 2, 3, 8, 17, 5, 10, 8, 16)       # an 8x17 crop at (2, 3) of a 10x20 image: flush right and bottom
    ok = dict(src=one, nbytes=600, N=1, tab=_table([row]), H=8, W=16, mean=mean, std=std, pad=pad, dst=one)

    def call(**kw):
        a = dict(ok, **kw)
        return f(None, a["src"], a["nbytes"], a["N"], a["tab"], a["H"], a["W"], a["mean"], a["std"], a["pad"], 0.0,
                 a["dst"], None)

    def with_(**cols):
        names = ("off", "Hi", "Wi", "y0", "x0", "Hc", "Wc", "Hr", "Wr", "Hp", "Wp")
        r = list(row)
        for k, v in cols.items():
            r[names.index(k)] = v
        return _table([tuple(r)])

    for name in ("src", "dst", "tab", "mean", "std", "pad"):
        assert call(**{name: None}) == E_BADARG, name
    # the crop
    assert call(tab=with_(y0=-1)) == E_BADARG
    assert call(tab=with_(x0=-1)) == E_BADARG
    assert call(tab=with_(Hc=0)) == E_BADARG
    assert call(tab=with_(Wc=0)) == E_BADARG
    assert call(tab=with_(Hc=-8)) == E_BADARG
    assert call(tab=with_(y0=3)) == E_BADARG                          # y0 + H_crop = 11 > 10
    assert call(tab=with_(x0=4)) == E_BADARG                          # x0 + W_crop = 21 > 20
    assert call(tab=with_(Hc=9)) == E_BADARG
    assert call(tab=with_(Wc=18)) == E_BADARG
    assert call(tab=with_(y0=2 ** 62, Hc=2 ** 62)) == E_BADARG        # no wrap-around in the sum
    assert call(tab=with_(x0=11)) == E_BADARG
    assert call(N=2, tab=_table([row, row[:3] + (3,) + row[4:]])) == E_BADARG
    # everything else as the batch entry
    assert call(N=0) == E_BADARG
    assert call(H=0) == E_BADARG
    assert call(N=33, tab=_table([row] * 33)) == E_TOO_LARGE
    assert call(H=65536) == E_TOO_LARGE
    assert call(std=(ctypes.c_float * 3)(1, 0, 1)) == E_BADARG
    assert call(pad=(ctypes.c_int * 3)(0, 256, 0)) == E_BADARG
    assert call(H=7) == E_BADARG
    assert call(tab=with_(Hr=9)) == E_BADARG                          # H_resized > H_pad
    assert call(nbytes=599) == E_BADARG                               # the IMAGE must lie in the buffer
    assert call(tab=with_(off=-1)) == E_BADARG
    assert call(tab=with_(Hi=40000, Wi=1, x0=0, Wc=1), nbytes=120000) == E_TOO_LARGE


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_slice_merge_rejects_bad_arguments(lib, suffix):
    f = getattr(lib, "codetr_slice_merge_" + suffix)
    one = ctypes.c_void_p(16)

    def call(ptrs=None, R=7, N=2, V=5, Q=300, metric=1, mode=1, thr=0.5, agnostic=0, keep=100):
        b, s, l, c, r, o, z, bo, so, lo, io, co = ptrs or [one] * 12
        return f(None, b, s, l, c, r, o, z, R, N, V, Q, metric, mode, thr, agnostic, keep, bo, so, lo, io, co)

    for i in range(12):
        ptrs = [one] * 12
        ptrs[i] = None
        assert call(ptrs) == E_BADARG, i
    for name in ("R", "N", "V", "Q"):
        assert call(**{name: 0}) == E_BADARG, name
        assert call(**{name: -3}) == E_BADARG, name
    assert call(metric=2) == E_BADARG
    assert call(metric=-1) == E_BADARG
    assert call(mode=2) == E_BADARG
    assert call(mode=-1) == E_BADARG
    assert call(thr=float("nan")) == E_BADARG
    assert call(thr=float("inf")) == E_BADARG
    assert call(V=65, Q=1) == E_TOO_LARGE                            # CODETR_SLICE_MAX_VIEWS
    assert call(V=1, Q=4097) == E_TOO_LARGE                          # V * Q = 4097
    assert call(V=14, Q=300) == E_TOO_LARGE                          # 4200
    assert call(V=64, Q=65) == E_TOO_LARGE
