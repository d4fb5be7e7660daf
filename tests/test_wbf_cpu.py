"""CPU: weighted boxes fusion -- known answers of the restatement (tests/wbf_ref.py), its agreement with a literal float64
transcription of the published algorithm, how `wbf_settings` / `tta_settings` / `Inferencer(tta=dict(wbf=...),
ensemble=...)` read their arguments, the header and its binding, and the argument contract of codetr_wbf_merge_*
(include/codetr_wbf.h), whose rejections happen on the host before any HIP call."""
import ctypes
import glob
import os

import numpy as np
import pytest

import wbf_ref as R
from conftest import ROOT

E_BADARG, E_TOO_LARGE = -1, -3
F = np.float32
CONFIGS = sorted(glob.glob(os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_*.py")))


def _views(rows):
    """[(view, box, score, label)] -> one-image operands, every view padded to the longest"""
    V = 1 + max(r[0] for r in rows)
    per = [[r for r in rows if r[0] == v] for v in range(V)]
    Q = max(len(p) for p in per)
    boxes, scores, labels = np.zeros((V, Q, 4), F), np.zeros((V, Q), F), np.zeros((V, Q), np.int64)
    for v, p in enumerate(per):
        for j, (_, b, s, l) in enumerate(p):
            boxes[v, j], scores[v, j], labels[v, j] = b, s, l
    return boxes, scores, labels, np.array([len(p) for p in per]), [False] * V, 100.0


# ---- 1. known answers ---------------------------------------------------------------------------------------------------
def test_two_views_of_one_object_fuse_into_their_weighted_mean():
    bx, sc, lab, c, n = R.fuse(*_views([(0, (0, 0, 10, 10), 0.9, 7), (1, (1, 1, 11, 11), 0.6, 7)]), iou_threshold=0.55)
    assert c.tolist() == [0] and n.tolist() == [2] and lab.tolist() == [7]
    assert bx[0].tolist() == [F(0.4), F(0.4), F(10.400001), F(10.400001)]
    assert sc[0] == F(0.75)
    # the same by the header's operations: IoU 81 / 119 > 0.55; SX1 = 0.9 * 0 + 0.6 * 1, SC = 0.9 + 0.6
    SC = F(F(0.9) + F(0.6))
    assert bx[0, 0] == F(F(F(0.9) * F(0)) + F(F(0.6) * F(1))) / SC
    assert bx[0, 2] == F(F(F(0.9) * F(10)) + F(F(0.6) * F(11))) / SC
    assert sc[0] == F(F(F(SC / F(2)) * F(2)) / F(2))


def test_a_lone_box_is_scaled_by_the_views_that_missed_it():
    ops = list(_views([(0, (50, 50, 60, 60), 0.8, 1), (1, (0, 0, 1, 1), 0.0, 1)]))
    ops[3] = np.array([1, 0])                                   # view 1 saw nothing
    bx, sc, lab, c, n = R.fuse(*ops)
    assert c.tolist() == [0] and n.tolist() == [1] and bx[0].tolist() == [50, 50, 60, 60]
    assert sc[0] == F(F(F(F(0.8) / F(1)) * F(1)) / F(2)) == F(0.4)


def test_equal_overlaps_go_to_the_lower_founder():
    """founders (0,0,10,10) and (4,0,14,10): mutual IoU 60 / 140, they stay apart; (2,0,12,10) has IoU 80 / 120 with
    both.  The later founder has the higher confidence here, so the package's first-created cluster would be the other.
    (Scores with few bits: conf * x / conf is x exactly, so the two overlaps are one fp32 value.)"""
    rows = [(0, (0, 0, 10, 10), 0.5, 3), (0, (4, 0, 14, 10), 0.75, 3), (1, (2, 0, 12, 10), 0.375, 3)]
    bx, sc, lab, c, n = R.fuse(*_views(rows), iou_threshold=0.55)
    assert sorted(zip(c.tolist(), n.tolist())) == [(0, 2), (1, 1)]
    assert c.tolist() == [0, 1] and sc.tolist() == [0.4375, 0.375]      # (0.5 + 0.375) / 2 > 0.75 / 2
    assert bx[0, 0] == F(0.75) / F(0.875) and bx[1].tolist() == [4, 0, 14, 10]


def test_conf_type_max_with_weights():
    rows = [(0, (0, 0, 10, 10), 0.5, 2), (1, (0, 0, 10, 10), 0.9, 2), (1, (50, 50, 60, 60), 0.4, 2)]
    bx, sc, lab, c, n = R.fuse(*_views(rows), weights=[2, 1], conf_type="max")
    # confs 1.0 (c 0), 0.9, 0.4; the cluster of c 0 has top 1.0, the lone box 0.4; wmax = 2
    assert c.tolist() == [0, 3] and n.tolist() == [2, 1]
    assert sc.tolist() == [F(F(F(0.5) * F(2)) / F(2)), F(F(0.4) / F(2))]
    assert bx[0].tolist() == [0, 0, 10, 10]
    bx, sc, lab, c, n = R.fuse(*_views(rows), weights=[2, 1], conf_type="avg")
    wsum = F(3)
    assert sc[0] == F(F(F(F(F(1.0) + F(0.9)) / F(2)) * F(2)) / wsum)


def test_reference_rules():
    rows = [(0, (0, 0, 10, 10), 0.9, 1), (0, (0, 0, 10, 10), 0.0, 1), (0, (0, 0, 10, 10), np.nan, 1),
            (1, (0, 0, 10, 10), 0.2, 1), (1, (0, 0, 10, 10), 0.6, 2)]
    bx, sc, lab, c, n = R.fuse(*_views(rows))
    assert c.tolist() == [0, 4] and n.tolist() == [2, 1] and lab.tolist() == [1, 2]     # zero and NaN scores are dropped
    assert R.fuse(*_views(rows), skip_box_thr=0.3)[4].tolist() == [1, 1]                 # 0.2 is skipped
    assert R.fuse(*_views(rows), max_keep=1)[3].tolist() == [0]
    # an IoU equal to the threshold does not join (81 / 119 is no fp32 tie: use boxes with IoU exactly 0.5)
    rows = [(0, (0, 0, 2, 2), 0.5, 1), (1, (0, 0, 2, 1), 0.25, 1)]
    assert R.fuse(*_views(rows), iou_threshold=0.5)[4].tolist() == [1, 1]
    assert R.fuse(*_views(rows), iou_threshold=0.49)[4].tolist() == [2]
    # un-flip before anything else
    b, s, l, cnt, _, w = _views([(0, (10, 20, 40, 60), 0.9, 3), (1, (60, 20, 90, 60), 0.8, 3)])
    assert R.fuse(b, s, l, cnt, [False, True], w)[4].tolist() == [2]
    assert R.fuse(b, s, l, cnt, [False, False], w)[4].tolist() == [1, 1]
    # more members than wsum: the score stops growing with n (votes > V)
    rows = [(0, (0, 0, 10, 10), 0.5, 1)] * 3
    bx, sc, lab, c, n = R.fuse(*_views(rows))
    assert n.tolist() == [3] and sc[0] == F(F(F(F(1.5) / F(3)) * F(1)) / F(1))


# ---- 2. against a literal float64 transcription of the published algorithm -----------------------------------------------
def _iou64(a, b):
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = w * h
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def wbf_literal(boxes, scores, labels, count, weights, thr, conf_type):
    """`ensemble_boxes.weighted_boxes_fusion` (conf_type 'avg' / 'max', allows_overflow=False) as published, in float64:
    per label the boxes in descending confidence; find_matching_box = the arg-max over the cluster list of the IoU with
    each fused box, above thr; the members of the chosen cluster are summed again at every step.  Two places follow
    this library's stated rule where the package leaves the order open or differs: equal confidences go in ascending c
    (the package's argsort leaves ties to the sort), and the output ties go by founder c.
    -> ([(founder c, votes, box, score)] in output order, the least |IoU - thr| met)"""
    V, Q = scores.shape
    w = np.ones(V) if weights is None else np.asarray(weights, np.float64)
    rows, margin = [], np.inf
    cands = [(v * Q + j, float(scores[v, j]) * w[v], boxes[v, j].astype(np.float64), int(labels[v, j]))
             for v in range(V) for j in range(int(count[v]))]
    for lab in sorted({c[3] for c in cands}):
        members, founders, fused = [], [], []
        for c, cf, b, _ in sorted((c for c in cands if c[3] == lab), key=lambda t: (-t[1], t[0])):
            best, bi = thr, -1
            for i, f in enumerate(fused):
                iou = _iou64(f, b)
                margin = min(margin, abs(iou - thr))
                if iou > best:
                    best, bi = iou, i
            if bi < 0:
                members.append([(cf, b)])
                founders.append(c)
                fused.append(b.copy())
            else:
                members[bi].append((cf, b))
                fused[bi] = sum(m[0] * m[1] for m in members[bi]) / sum(m[0] for m in members[bi])
        for mem, c, f in zip(members, founders, fused):
            n = len(mem)
            if conf_type == "max":
                sc = max(m[0] for m in mem) / w.max()
            else:
                sc = sum(m[0] for m in mem) / n * min(n, w.sum()) / w.sum()
            rows.append((c, n, f, sc))
    rows.sort(key=lambda r: (-r[3], r[0]))
    return rows, margin


def _scene(seed):
    """the issue's generator: 50 objects of 4 labels seen by 6 views with probability 0.8, jittered by 3 px"""
    rng = np.random.default_rng(seed)
    n_obj, V = 50, 6
    corner = rng.uniform(0, 900, (n_obj, 2))
    size = rng.uniform(20, 160, (n_obj, 2))
    truth = np.concatenate([corner, corner + size], 1)
    obj_label = rng.integers(0, 4, n_obj)
    boxes, scores, labels = np.zeros((V, n_obj, 4), F), np.zeros((V, n_obj), F), np.zeros((V, n_obj), np.int64)
    count = np.zeros(V, np.int64)
    for v in range(V):
        keep = np.flatnonzero(rng.random(n_obj) < 0.8)
        k = len(keep)
        b = np.abs(truth[keep] + rng.normal(0, 3, (k, 4)))
        boxes[v, :k] = b.astype(np.float16).astype(F)
        scores[v, :k] = rng.uniform(0.05, 1, k).astype(np.float16).astype(F)
        labels[v, :k] = obj_label[keep]
        count[v] = k
    return boxes, scores, labels, count


@pytest.mark.parametrize("conf_type", ["avg", "max"])
@pytest.mark.parametrize("seed", range(6))
def test_restatement_agrees_with_the_literal_transcription(seed, conf_type):
    boxes, scores, labels, count = _scene(seed)
    weights = None if seed % 2 == 0 else [2, 1, 1, 0.5, 1, 1]
    thr = 0.55
    lit, margin = wbf_literal(boxes, scores, labels, count, weights, thr, conf_type)
    # the precondition (a condition, not a measurement): no decision of the float64 run is within fp32's reach
    assert margin > 1e-4, f"seed {seed}: an IoU lies {margin:.2e} from the threshold"
    bx, sc, lab, c, n = R.fuse(boxes, scores, labels, count, [False] * 6, 1000.0, weights=weights, conf_type=conf_type,
                               iou_threshold=thr)
    assert len(lit) > 40 and max(r[1] for r in lit) >= 4
    assert c.tolist() == [r[0] for r in lit]                    # founders and the output order
    assert n.tolist() == [r[1] for r in lit]                    # votes
    worst = 0.0
    for i, (_, votes, f, s) in enumerate(lit):
        # n rounded products and sums of non-negative terms and one division: no cancellation
        bound = (votes + 4) * 2.0 ** -24
        err = max(np.max(np.abs(bx[i].astype(np.float64) - f) / f), abs(float(sc[i]) - s) / s)
        worst = max(worst, err / bound)
        assert err <= bound, (seed, i, votes, err, bound)
    print(f"seed {seed} {conf_type}: margin {margin:.2e}, {len(lit)} clusters, worst error / bound {worst:.3f}")


# ---- 3. settings ------------------------------------------------------------------------------------------------------
def test_wbf_settings():
    from codetr.hip_ops import wbf_settings

    assert wbf_settings(None) == wbf_settings({}) == dict(iou_threshold=0.55, skip_box_thr=0.0, conf_type="avg", weights=None)
    w = wbf_settings(dict(iou_threshold=0.6, skip_box_thr=0.1, conf_type="max", weights=(2, 1)))
    assert w == dict(iou_threshold=0.6, skip_box_thr=0.1, conf_type="max", weights=[2.0, 1.0])
    with pytest.raises(ValueError, match="iou_thr"):
        wbf_settings(dict(iou_thr=0.5))                         # ensemble_boxes' spelling is the function's, not the dict's
    for kind in ("box_and_model_avg", "absent_model_aware_avg"):
        with pytest.raises(NotImplementedError):
            wbf_settings(dict(conf_type=kind))
    for bad in (dict(conf_type="median"), dict(iou_threshold=float("nan")), dict(skip_box_thr=float("inf")),
                dict(weights=[1, 0]), dict(weights=[1, -2]), dict(weights=[float("nan")]), dict(weights=[])):
        with pytest.raises(ValueError):
            wbf_settings(bad)
    with pytest.raises(ValueError):
        wbf_settings("avg")


def test_tta_settings_take_the_wbf_key():
    from codetr.inferencer import tta_settings

    t = tta_settings(None, dict(scales=[(640, 480)], flip=True, wbf=dict(conf_type="max"), max_per_img=50))
    assert t["nms"] is None and t["max_per_img"] == 50 and len(t["views"]) == 2
    assert t["wbf"] == dict(iou_threshold=0.55, skip_box_thr=0.0, conf_type="max", weights=None)
    assert tta_settings(None, dict(scales=[(640, 480)], wbf={}))["wbf"]["conf_type"] == "avg"
    # every existing dict is read as before, with None under the new key
    t = tta_settings(None, dict(scales=[(640, 480)], nms=dict(type="nms", iou_threshold=0.6)))
    assert t["wbf"] is None and t["nms"] == dict(type="nms", iou_threshold=0.6, method="linear", min_score=1e-3)
    assert tta_settings(None, dict(scales=[(640, 480)], wbf=None))["nms"]["type"] == "nms"
    with pytest.raises(ValueError, match="one of them"):
        tta_settings(None, dict(scales=[(640, 480)], nms=dict(type="nms"), wbf={}))
    with pytest.raises(NotImplementedError, match="wbf=dict"):
        tta_settings(None, dict(scales=[(640, 480)], nms=dict(type="wbf")))
    with pytest.raises(ValueError):
        tta_settings(None, dict(scales=[(640, 480)], wbf=dict(threshold=0.5)))
    with pytest.raises(NotImplementedError):
        tta_settings(None, dict(scales=[(640, 480)], wbf=dict(conf_type="box_and_model_avg")))
    with pytest.raises(ValueError):
        tta_settings(None, dict(scales=[(640, 480)], wbf={}, fusion="wbf"))


def test_inferencer_constructor_takes_wbf_and_ensemble():
    from codetr.inferencer import Inferencer

    cfg = [c for c in CONFIGS if "swin_l" in c][0]
    plain = Inferencer(None, cfg, dataset_meta=None)
    assert plain.tta is None and plain.ensemble == []            # the defaults: nothing changes
    inf = Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(320, 200)], flip=True, wbf={}))
    assert inf.tta["nms"] is None and inf.tta["wbf"]["iou_threshold"] == 0.55 and inf.ensemble == []
    other = object()
    inf = Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(320, 200), (640, 400)], flip=True,
                                                            wbf=dict(weights=[2, 1])), ensemble=[other])
    assert inf.ensemble == [other]
    assert inf.tta["wbf"]["weights"] == [2.0] * 4 + [1.0] * 4   # one per model -> one per view, v = (k * S + s) * F + f
    inf = Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(320, 200)], wbf=dict(weights=[3, 1])), ensemble=[other])
    assert inf.tta["wbf"]["weights"] == [3.0, 1.0]              # (one per view and one per model are the same here)
    inf = Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(320, 200)], nms=dict(type="nms")), ensemble=[other])
    assert inf.tta["wbf"] is None and inf.ensemble == [other]   # an ensemble merged by NMS
    with pytest.raises(ValueError, match="tta"):
        Inferencer(None, cfg, dataset_meta=None, ensemble=[other])
    with pytest.raises(ValueError, match="weights"):
        Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(320, 200)], flip=True, wbf=dict(weights=[1, 2, 3])),
                   ensemble=[other])
    with pytest.raises(ValueError, match="weights"):
        Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(320, 200)], flip=True, wbf=dict(weights=[1, 2, 3])))
    with pytest.raises(ValueError, match="16"):
        Inferencer(None, cfg, dataset_meta=None, tta=dict(scales=[(100 + i, 50) for i in range(5)], flip=True, wbf={}),
                   ensemble=[other])


# ---- 4. the header and its binding -------------------------------------------------------------------------------------
def test_header_parses_and_the_table_equals_its_declarations():
    from codetr import _cabi, _cheader, _wbf, hip_ops

    text = open(os.path.join(ROOT, "include", "codetr_wbf.h")).read()
    functions, defines = _cheader.parse(text)
    assert list(functions) == ["codetr_wbf_abi_version", "codetr_wbf_merge_f16", "codetr_wbf_merge_bf16",
                               "codetr_wbf_merge_f32"]
    assert defines == dict(CODETR_WBF_ABI_VERSION=1, CODETR_WBF_MAX_CANDIDATES=4096, CODETR_WBF_CONF_AVG=0,
                           CODETR_WBF_CONF_MAX=1)
    assert set(_wbf.SIGNATURES) == set(functions) and _wbf.CONF_TYPES == dict(avg=0, max=1)
    assert hip_ops.WBF_MAX_CANDIDATES == 4096 and _cabi.ABI_VERSION == 54
    i, l, p, u, f = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    assert _wbf.SIGNATURES["codetr_wbf_abi_version"] == (i, [])
    tta = _cheader.functions["codetr_tta_merge_f16"][1]
    for suffix in ("f16", "bf16", "f32"):
        assert _wbf.SIGNATURES["codetr_wbf_merge_" + suffix] == (i, [p, p, p, p, p, l, l, l, u, p, p, i, f, f, l] + [p] * 6)
        params = functions["codetr_wbf_merge_" + suffix][1]
        # codetr_tta_merge_*'s operands, the WBF parameters in place of its mode .. max_keep, its outputs, the votes
        assert params[:10] == tta[:10] and params[15:20] == tta[14:] and params[14] == tta[13]
        assert [n for _, n in params[10:14]] == ["weights_host", "conf_type", "iou_threshold", "skip_box_thr"]
        assert params[20] == ("int *", "votes_out_dev")
    assert not set(functions) & set(_cabi.SIGNATURES)           # a companion: codetr_hip.h and its version are untouched
    for phrase in ("PARITY IS UNPINNED", "the tie rule", "score * weight > 0", "never contracted",
                   "((SC / (float)n) * fminf((float)n, wsum)) / wsum", "top / wmax"):
        assert phrase in text, phrase


@pytest.fixture
def lib():
    from codetr import _cabi, _wbf

    _cabi.RECORDER = []
    try:
        yield _wbf.load()
        assert _cabi.RECORDER == []
    finally:
        _cabi.RECORDER = None


def test_abi_version(lib):
    from codetr import _cabi

    assert lib.codetr_wbf_abi_version() == 1 and "wbf_merge" in _cabi.CALLS


def reject_cases(f):
    """every rejection of codetr_wbf_merge_* -> [(what, returned code, expected code)]; the pointers are never read"""
    one = ctypes.c_void_p(16)

    def call(ptrs=None, V=2, N=3, Q=300, flip=0b10, weights=None, conf=0, iou=0.55, skip=0.0, keep=100):
        b, s, l, c, w, bo, so, lo, io, co, vo = ptrs or [one] * 11
        wt = None if weights is None else (ctypes.c_float * len(weights))(*weights)
        return f(None, b, s, l, c, V, N, Q, flip, w, wt, conf, iou, skip, keep, bo, so, lo, io, co, vo)

    out = []
    for i in range(11):
        ptrs = [one] * 11
        ptrs[i] = None
        out.append((f"null pointer {i}", call(ptrs), E_BADARG))
    inf, nan = float("inf"), float("nan")
    for what, kw, code in [
            ("V = 0", dict(V=0), E_BADARG), ("N = 0", dict(N=0), E_BADARG), ("Q = 0", dict(Q=0), E_BADARG),
            ("Q < 0", dict(Q=-5), E_BADARG), ("flip bit at V", dict(flip=0b100), E_BADARG),
            ("flip bit above V = 1", dict(V=1, Q=10, flip=0b10), E_BADARG), ("conf_type 2", dict(conf=2), E_BADARG),
            ("conf_type -1", dict(conf=-1), E_BADARG), ("iou nan", dict(iou=nan), E_BADARG), ("iou inf", dict(iou=inf), E_BADARG),
            ("skip nan", dict(skip=nan), E_BADARG), ("skip -inf", dict(skip=-inf), E_BADARG),
            ("weight 0", dict(weights=[1, 0]), E_BADARG), ("weight < 0", dict(weights=[-1, 1]), E_BADARG),
            ("weight nan", dict(weights=[1, nan]), E_BADARG), ("weight inf", dict(weights=[inf, 1]), E_BADARG),
            ("17 views", dict(V=17, Q=1, flip=0), E_TOO_LARGE), ("4097 candidates", dict(V=1, Q=4097, flip=0), E_TOO_LARGE),
            ("7 x 586", dict(V=7, Q=586, flip=0), E_TOO_LARGE), ("16 x 257", dict(V=16, Q=257, flip=0), E_TOO_LARGE)]:
        out.append((what, call(**kw), code))
    return out


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_wbf_merge_rejects_bad_arguments(lib, suffix):
    for what, got, want in reject_cases(getattr(lib, "codetr_wbf_merge_" + suffix)):
        assert got == want, what
