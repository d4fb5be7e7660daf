"""GPU: codetr_postprocess_softnms_* (csrc/prepost.hip) against the numpy fp32 reference of its stated semantics
(tests/softnms_ref.py) -- boxes, scores, labels, index and count bit for bit, zero rows beyond count -- then
hip_ops.soft_nms and the soft mode of `Inferencer` on stub models.

One exception to "bit for bit": where the reference's score is a NaN the kernel's must be a NaN; which NaN a conversion
to f16 / bf16 produces (sign, payload) is not part of the semantics."""
import os

import numpy as np
import pytest
import torch

import softnms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIN = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
QS = [1, 63, 64, 65, 300, 1024]   # one lane, either side of a wave, the workload, the full workgroup
_BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
DIVS = [(0.6, 0.6, 0.6, 0.6), (1152 / 1919, 768 / 1281, 1152 / 1919, 768 / 1281), (1.7, 2.3, 1.7, 2.3)]
LAYOUTS = ("one", "eighty", "distinct", "mixed")


def _bits(t):
    return t.contiguous().view(_BITS[t.dtype]).cpu()


def _labels(rng, Q, layout):
    if layout == "one":                      # the longest single-wave chain: up to 16 elements per lane
        return np.full(Q, 17, np.int64)
    if layout == "eighty":
        return rng.integers(0, 80, Q)
    if layout == "distinct":                 # every segment of length 1 (and labels beyond 32 bits, negative ones)
        return rng.permutation(Q).astype(np.int64) * 3 - 40 + (np.arange(Q) % 2) * (1 << 40)
    lab = 1000 + np.arange(Q, dtype=np.int64)   # one label of 130 (more than two waves' worth) among singletons
    lab[rng.permutation(Q)[:min(130, max(1, Q // 2))]] = 5
    return lab


def _image(rng, Q, layout, clustered, dtype, min_score=1e-3):
    """one image's candidates in the storage type: (boxes [Q,4], scores [Q]) torch CPU tensors, labels numpy"""
    if clustered:                            # many IoUs >= 0.8, so that decays chain; coordinates small enough for bf16
        centres = rng.uniform(40, 200, (max(1, Q // 12), 2))
        c = centres[rng.integers(0, len(centres), Q)] + rng.uniform(-3, 3, (Q, 2))
        wh = 64 + rng.uniform(-4, 4, (Q, 2))
    else:
        c, wh = rng.uniform(0, 250, (Q, 2)), rng.uniform(2, 90, (Q, 2))
    boxes = np.concatenate((c - wh / 2, c + wh / 2), 1)
    scores = rng.uniform(0, 1, Q)
    scores[::7] *= 0.004                                             # either side of min_score before any decay
    if Q >= 8:
        boxes[Q // 2:Q // 2 + Q // 8] = boxes[:Q // 8]                # duplicated boxes (IoU 1: linear weight 0)
        scores[3::5] = scores[1]                                     # duplicated scores: the tie order
        boxes[5] = boxes[6] = (30, 30, 30, 50)                       # a zero-area pair
        scores[2] = min_score                                        # (rounded to the storage type below)
        scores[4] = 0.0
    return torch.from_numpy(boxes).to(dtype), torch.from_numpy(scores).to(dtype), _labels(rng, Q, layout)


def _run_and_compare(dtype, images, divs, iou, method, min_score=1e-3, thr=None, max_keep=None):
    """images: [(boxes, scores, labels)] of one Q -> launch once, compare every image with the reference"""
    from codetr import _cabi, hip_ops

    N, Q = len(images), images[0][1].numel()
    boxes = torch.stack([im[0] for im in images]).to(DEV)
    scores = torch.stack([im[1] for im in images]).to(DEV)
    labels = torch.from_numpy(np.stack([im[2] for im in images])).to(DEV)
    div = torch.tensor(divs[:N], dtype=torch.float64).to(dtype)
    before = dict(_cabi.CALLS)
    dets = hip_ops.postprocess_detections_soft(boxes, scores, labels, div.to(DEV), thr, iou, method, min_score, max_keep)
    assert _cabi.CALLS["postprocess_softnms"] == before["postprocess_softnms"] + 1
    assert _cabi.CALLS["postprocess_detections"] == before["postprocess_detections"]
    host = hip_ops.detections_to_host(dets)
    assert host.index.dtype == torch.int32 and host.index.shape == (N, Q) and host.boxes.dtype == dtype
    thr_t = None if thr is None else np.float32(torch.tensor(thr, dtype=torch.float64).to(dtype).float().item())
    to_storage = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)  # noqa: E731
    total = 0
    for i, (b, s, lab) in enumerate(images):
        eb, es, el, ei = R.postprocess(b.float().numpy(), s.float().numpy(), lab, div[i].float().numpy(), to_storage, iou,
                                       method, min_score, thr_t, max_keep or 0)
        c = int(host.count[i])
        print(f"image {i}: Q {Q} kept {c} expected {len(ei)}")
        assert c == len(ei), (i, c, len(ei))
        assert host.index[i, :c].tolist() == ei.tolist(), i
        assert host.labels[i, :c].tolist() == el.tolist(), i
        nan = torch.isnan(es.float())
        assert torch.equal(torch.isnan(host.scores[i, :c].float()), nan), i
        assert torch.equal(_bits(host.scores[i, :c])[~nan], _bits(es)[~nan]), i
        assert torch.equal(_bits(host.boxes[i, :c]), _bits(eb)), i
        assert bool((_bits(host.scores[i, c:]) == 0).all()) and bool((_bits(host.boxes[i, c:]) == 0).all())
        assert bool((host.labels[i, c:] == 0).all()) and bool((host.index[i, c:] == 0).all())
        total += c
    return total, host


# ---- 1. the kernel against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q", QS)
def test_softnms_linear_matches_the_reference(dtype, Q):
    """N = 3; the label layout x box layout of each image rotates with the case, so every Q and dtype meets the long
    single-label chain, many labels, singletons and the mix, clustered and spread"""
    case = DTYPES.index(dtype) * len(QS) + QS.index(Q)
    rng = np.random.default_rng(100 + case)
    combos = [(3 * case + i) % 8 for i in range(3)]
    images = [_image(rng, Q, LAYOUTS[k // 2], k % 2 == 0, dtype) for k in combos]
    total, _ = _run_and_compare(dtype, images, DIVS, (0.8, 0.5)[case % 2], "linear")
    if Q >= 63:
        assert total < 3 * Q    # something fell under min_score


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_softnms_full_workgroup_every_label_layout(dtype, layout):
    """Q = 1024, N = 1: each label layout on clustered boxes, the single label being the worst case (one wave, up to
    1024 picks, 16 elements per lane)"""
    rng = np.random.default_rng(300 + LAYOUTS.index(layout))
    total, _ = _run_and_compare(dtype, [_image(rng, 1024, layout, True, dtype)], DIVS, 0.8, "linear")
    assert 0 < total < 1024


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q", [65, 300])
def test_softnms_naive_matches_the_reference(dtype, Q):
    rng = np.random.default_rng(500 + Q)
    for N, layout, clustered in ((1, "one", True), (3, "eighty", False), (1, "mixed", True)):
        images = [_image(rng, Q, layout, clustered, dtype) for _ in range(N)]
        _run_and_compare(dtype, images, DIVS, 0.8 if clustered else 0.3, "naive")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_thr", [False, True])
def test_softnms_threshold_and_nan_scores(dtype, with_thr):
    """threshold on: scores equal to the threshold at storage precision and one ulp either side, NaNs fail it; off: a NaN
    with the sign bit clear is the highest score, one with it set the lowest"""
    rng = np.random.default_rng(700 + with_thr)
    thr = 0.3
    images = []
    for i, layout in enumerate(("eighty", "one", "mixed")):
        b, s, lab = _image(rng, 300, layout, i != 0, dtype)
        t = torch.tensor(thr, dtype=torch.float64).to(dtype).reshape(1)
        tb = t.view(_BITS[dtype])
        for k, v in enumerate((t, (tb + 1).view(dtype), (tb - 1).view(dtype))):
            s[40 + 9 * k] = s[100 + k] = v[0]
        s[20 + i] = s[150] = float("nan")
        s[60 + i] = -float("nan")
        lab[150] = lab[60 + i]                # a NaN of either sign inside one label
        images.append((b, s, lab))
    total, host = _run_and_compare(dtype, images, DIVS, 0.8, "linear", thr=thr if with_thr else None)
    assert bool(torch.isnan(host.scores.float()).any()) != with_thr


@pytest.mark.parametrize("max_keep", [0, 1, 100, 300])
def test_softnms_max_keep(max_keep):
    rng = np.random.default_rng(900)
    images = [_image(rng, 300, "eighty", False, torch.float16), _image(rng, 300, "one", True, torch.float16)]
    total, host = _run_and_compare(torch.float16, images, DIVS, 0.8, "linear", max_keep=max_keep)
    if max_keep in (1, 100):
        assert int(host.count[0]) == max_keep and 0 < int(host.count[1]) <= max_keep


def test_softnms_min_score_variants_and_unit_divisors():
    """a larger min_score (more drops after decay), min_score 0 (nothing ever leaves; 0 and -0 scores stay) and unit
    divisors (boxes come back unchanged)"""
    rng = np.random.default_rng(1000)
    for dtype in DTYPES:
        images = [_image(rng, 300, "mixed", True, dtype, 0.05), _image(rng, 300, "eighty", True, dtype, 0.05)]
        _run_and_compare(dtype, images, DIVS, 0.5, "linear", min_score=0.05)
        total, host = _run_and_compare(dtype, images, [(1.0,) * 4] * 2, 0.5, "linear", min_score=0.0)
        assert total == 600
        order = host.index[0].long()
        assert torch.equal(_bits(host.boxes[0]), _bits(images[0][0][order]))


def test_iou_equal_to_the_threshold_decays_on_the_gpu():
    """`>=`: IoU exactly 0.5 at threshold 0.5 decays (linear) / removes (naive); one ulp above the IoU it does not"""
    from codetr import hip_ops

    boxes = torch.tensor([[0, 0, 10, 10], [0, 0, 10, 5], [40, 40, 50, 50]], dtype=torch.float32, device=DEV)
    scores = torch.tensor([0.9, 0.5, 0.7], dtype=torch.float32, device=DEV)
    labels = torch.zeros(3, dtype=torch.int64, device=DEV)
    s, keep = hip_ops.soft_nms(boxes, scores, labels, 0.5)
    assert keep.tolist() == [0, 2, 1] and s.tolist() == [np.float32(0.9), np.float32(0.7), 0.25]
    s, keep = hip_ops.soft_nms(boxes, scores, labels, 0.5, method="naive")
    assert keep.tolist() == [0, 2]
    s, keep = hip_ops.soft_nms(boxes, scores, labels, float(np.nextafter(np.float32(0.5), np.float32(1))))
    assert keep.tolist() == [0, 2, 1] and s.tolist() == [np.float32(0.9), np.float32(0.7), 0.5]


def test_ties_go_to_the_lowest_index_on_the_gpu():
    """equal scores on equal boxes: the lower query index is picked (undecayed), the higher one decayed by 1 - 1 = 0"""
    from codetr import hip_ops

    box = [10.0, 10.0, 50.0, 50.0]
    boxes = torch.tensor([box, box, [12.0, 10.0, 52.0, 50.0], [12.0, 10.0, 52.0, 50.0]], dtype=torch.float32, device=DEV)
    scores = torch.tensor([0.5, 0.5, 0.25, 0.25], dtype=torch.float32, device=DEV)
    labels = torch.tensor([1, 1, 2, 3], device=DEV)
    s, keep = hip_ops.soft_nms(boxes, scores, labels, 0.8, min_score=0.0)
    assert keep.tolist() == [0, 2, 3, 1] and s.tolist() == [0.5, 0.25, 0.25, 0.0]


# ---- 2. hip_ops.soft_nms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_soft_nms_is_the_single_image_launch(dtype):
    from codetr import _cabi, hip_ops

    rng = np.random.default_rng(1100)
    b, s, lab = _image(rng, 200, "eighty", True, dtype)
    labels = torch.from_numpy(lab % 4).to(DEV)
    before = _cabi.CALLS["postprocess_softnms"]
    new_scores, keep = hip_ops.soft_nms(b.to(DEV), s.to(DEV), labels, 0.6, "linear", 0.01)
    assert _cabi.CALLS["postprocess_softnms"] == before + 1
    one = torch.ones((1, 4), dtype=dtype, device=DEV)
    host = hip_ops.detections_to_host(hip_ops.postprocess_detections_soft(b.to(DEV)[None], s.to(DEV)[None], labels[None],
                                                                           one, None, 0.6, "linear", 0.01))
    c = int(host.count[0])
    assert 0 < c < 200 and keep.dtype == torch.int64 and new_scores.dtype == dtype
    assert keep.tolist() == host.index[0, :c].tolist()
    assert torch.equal(_bits(new_scores), _bits(host.scores[0, :c]))
    ei, es = R.soft_nms(b.float().numpy(), s.float().numpy(), (lab % 4), 0.6, "linear", 0.01)
    assert keep.tolist() == ei.tolist()
    assert torch.equal(_bits(new_scores), _bits(torch.from_numpy(es).to(dtype)))


def test_soft_nms_empty_too_large_and_unknown_method():
    from codetr import _cabi, hip_ops

    before = _cabi.CALLS["postprocess_softnms"]
    s, keep = hip_ops.soft_nms(torch.empty((0, 4), device=DEV), torch.empty((0,), device=DEV),
                               torch.empty((0,), dtype=torch.int64, device=DEV), 0.8)
    assert s.shape == (0,) and keep.shape == (0,) and keep.dtype == torch.int64 and s.dtype == torch.float32
    big = torch.zeros((1025, 4), device=DEV)
    with pytest.raises(ValueError, match="1024"):
        hip_ops.soft_nms(big, big[:, 0], big[:, 0].long(), 0.8)
    with pytest.raises(NotImplementedError, match="gaussian"):
        hip_ops.soft_nms(big[:4], big[:4, 0], big[:4, 0].long(), 0.8, method="gaussian")
    with pytest.raises(ValueError, match="quadratic"):
        hip_ops.soft_nms(big[:4], big[:4, 0], big[:4, 0].long(), 0.8, method="quadratic")
    assert _cabi.CALLS["postprocess_softnms"] == before   # none of these launched


# ---- 3. Inferencer, stub models -------------------------------------------------------------------------------------------
def _soft_inferencer(model, **kw):
    from codetr.inferencer import Inferencer

    return Inferencer(model, SWIN, dataset_meta=None, **kw)


def _expected_soft(inf, images, dtype, model):
    """the reference's detections for every image from the stub model's raw predictions"""
    out = []
    to_storage = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)  # noqa: E731
    thr = inf.score_threshold if inf.score_threshold > 0 else None
    thr_t = None if thr is None else np.float32(torch.tensor(thr, dtype=torch.float64).to(dtype).float().item())
    for img in images:
        x, m, metas = inf.preprocess_batch([img], DEV, dtype)
        b, s, lab = (t[0].cpu() for t in model(x, m))
        sf = metas[0]["scale_factor"]
        div = torch.tensor([sf[0], sf[1]] * 2, dtype=dtype).float().numpy()
        eb, es, el, _ = R.postprocess(b.float().numpy(), s.float().numpy(), lab.numpy(), div, to_storage, inf.iou_threshold,
                                      inf.soft_method, inf.min_score, thr_t, inf.max_per_img or 0)
        out.append({"labels": el.tolist(), "scores": es.float().tolist(), "bboxes": eb.float().tolist()})
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_soft_mode_of_the_inferencer_with_a_stub_model(dtype):
    from codetr import _cabi
    from test_inferencer_batch_gpu import _images, _row_model, _same

    seen = []
    model = _row_model(seen)
    inf = _soft_inferencer(model, nms_type="config", score_threshold=0.3)
    assert inf.soft and inf.max_per_img == 300
    images = _images([(480, 640), (1333, 2000), (37, 53), (768, 1152), (600, 900)], 13)
    expect = _expected_soft(inf, images, dtype, model)
    assert sum(len(p["labels"]) for p in expect) > 10
    seen.clear()
    for bs, chunks in ((1, 5), (4, 2)):
        before = dict(_cabi.CALLS)
        got = inf(images, device=DEV, dtype=dtype, batch_size=bs)["predictions"]
        assert _cabi.CALLS["postprocess_softnms"] - before["postprocess_softnms"] == chunks      # one launch per chunk
        assert _cabi.CALLS["preprocess_batch"] - before["preprocess_batch"] == chunks            # the chunked path
        assert _cabi.CALLS["postprocess_detections"] == before["postprocess_detections"]
        assert _cabi.CALLS["batched_nms"] == before["batched_nms"] and _cabi.CALLS["preprocess"] == before["preprocess"]
        _same(got, expect)
    assert seen == [(1, 3, 768, 1152)] * 5 + [(4, 3, 768, 1152), (1, 3, 768, 1152)]
    # the per-image path (run_inference: hip_ops.soft_nms) agrees bit for bit with the chunked one
    per_image = []
    with torch.no_grad():
        for img in images:
            x, m, metas = inf.preprocess_batch([img], DEV, dtype)
            r = inf.run_inference(x, m, metas)[0]
            per_image.append({"labels": r["labels"].tolist(), "scores": r["scores"].float().tolist(),
                              "bboxes": r["bboxes"].float().tolist()})
    _same(per_image, expect)


def test_soft_mode_without_threshold_cuts_at_max_per_img():
    from test_inferencer_batch_gpu import _images, _row_model, _same

    model = _row_model([])
    inf = _soft_inferencer(model, nms_type="soft_nms")
    inf.max_per_img = 40
    assert inf.score_threshold == 0
    images = _images([(480, 640), (600, 900)], 21)
    expect = _expected_soft(inf, images, torch.float16, model)
    got = inf(images, device=DEV, dtype=torch.float16, batch_size=2)["predictions"]
    assert [len(p["labels"]) for p in got] == [40, 40]
    _same(got, expect)


@pytest.mark.parametrize("batch_size", [1, 4])
def test_default_inferencer_is_unchanged(batch_size):
    """nms_type=None: hard NMS, no cut -- what oracle/inferencer_ref.postprocess computes from the same predictions"""
    import inferencer_ref
    from codetr import _cabi
    from test_inferencer_batch_gpu import _images, _row_model

    model = _row_model([])
    inf = _soft_inferencer(model, score_threshold=0.3)
    assert not inf.soft and inf.max_per_img is None
    images = _images([(480, 640), (1333, 2000), (37, 53), (768, 1152), (600, 900)], 13)
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=torch.float32, batch_size=batch_size)["predictions"]
    assert _cabi.CALLS["postprocess_softnms"] == before["postprocess_softnms"]
    for img, p in zip(images, got):
        x, m, metas = inf.preprocess_batch([img], DEV, torch.float32)
        b, s, lab = (t[0].cpu().numpy() for t in model(x, m))
        eb, es, el = inferencer_ref.postprocess(b, s, lab, 0.3, 0.8, metas[0]["scale_factor"])
        assert p["labels"] == el.tolist() and len(el) > 0
        assert np.array_equal(np.asarray(p["scores"], np.float32), es)
        assert np.array_equal(np.asarray(p["bboxes"], np.float32).reshape(-1, 4), eb)
