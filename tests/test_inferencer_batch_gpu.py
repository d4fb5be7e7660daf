"""GPU: the batched Inferencer path (codetr_preprocess_batch_u8_*, codetr_postprocess_detections_*; csrc/prepost.hip)
against the per-image path it must reproduce -- hip_ops.preprocess_image + DetDataPreprocessor's divisor padding on the
way in, Inferencer.postprocess_predictions + run_inference's rescale on the way out -- bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIN = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")
R50 = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_r50_8xb2_1x_coco.py")
# 1x1, tall, wide, larger than the scale, odd sizes
SIZES = [(1, 1), (900, 120), (100, 1500), (2000, 3000), (37, 53), (333, 517)]
_BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _bits(t):
    return t.contiguous().view(_BITS[t.dtype]).cpu()


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _inferencer(model=None, cfg=SWIN, **attrs):
    from codetr.inferencer import Inferencer

    inf = Inferencer(model, cfg, dataset_meta=None)
    for k, v in attrs.items():
        setattr(inf, k, v)
    return inf


def _same(a, b):
    """two lists of prediction dicts are equal, NaN scores / coordinates included"""
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p["labels"] == q["labels"]
        for k in ("scores", "bboxes"):
            x, y = np.asarray(p[k], np.float64), np.asarray(q[k], np.float64)
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), k


# ---- 1. preprocessing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_size,divisor", [((1152, 768), 1), (None, 1), (None, 32), ((500, 300), 32)])
def test_preprocess_batch_matches_the_single_image_path(pad_size, divisor):
    from codetr import _cabi, hip_ops
    from codetr.inferencer import rescale_size

    inf = _inferencer(pad_size=pad_size, pad_size_divisor=divisor, pad_value=0.5, pad_val=(114, 7, 250))
    images = _images(SIZES, 11)
    expect = []
    for img in images:
        nh, nw = rescale_size(img.shape[0], img.shape[1], inf.scale)
        Hp, Wp = (nh, nw) if pad_size is None else (max(pad_size[1], nh), max(pad_size[0], nw))
        expect.append((nh, nw, Hp, Wp))
    rnd = lambda v: -(-v // divisor) * divisor  # noqa: E731
    Hb, Wb = max(rnd(e[2]) for e in expect), max(rnd(e[3]) for e in expect)
    results = {}
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        before = dict(_cabi.CALLS)
        x, m, metas = inf.preprocess_batch(images, DEV, dtype)
        assert _cabi.CALLS["preprocess_batch"] == before["preprocess_batch"] + 1
        assert _cabi.CALLS["preprocess"] == before["preprocess"]
        assert x.shape == (len(images), 3, Hb, Wb) and m.shape == (len(images), Hb, Wb) and x.dtype == m.dtype == dtype
        results[dtype] = (x, m)
        for i, (img, (nh, nw, Hp, Wp)) in enumerate(zip(images, expect)):
            assert metas[i]["img_shape"] == (nh, nw) and metas[i]["pad_shape"] == (rnd(Hp), rnd(Wp))
            assert metas[i]["batch_input_shape"] == (Hb, Wb)
            if dtype == torch.bfloat16:
                continue
            # inside the pipeline's Pad region: bit-identical to the single-image kernel
            xr, mr = hip_ops.preprocess_image(torch.from_numpy(img).to(DEV), (nh, nw), (Hp, Wp), inf.mean, inf.std,
                                              inf.pad_val, dtype)
            assert torch.equal(_bits(x[i, :, :Hp, :Wp]), _bits(xr)) and torch.equal(_bits(m[i, :Hp, :Wp]), _bits(mr))
            # beyond it: the raw pad_value, mask 1
            assert bool((x[i, :, Hp:, :] == 0.5).all()) and bool((x[i, :, :, Wp:] == 0.5).all())
            assert bool((m[i, Hp:, :] == 1).all()) and bool((m[i, :, Wp:] == 1).all())
            # and the whole per-image tensor of Inferencer.preprocess (which adds the divisor padding with F.pad)
            xs, ms, meta = inf.preprocess(img, DEV, dtype)
            Hd, Wd = meta["pad_shape"]
            assert (Hd, Wd) == metas[i]["pad_shape"]
            assert torch.equal(_bits(x[i, :, :Hd, :Wd]), _bits(xs[0])) and torch.equal(_bits(m[i, :Hd, :Wd]), _bits(ms[0]))
    # bf16: the f32 result rounded once
    x32, m32 = results[torch.float32]
    xb, mb = results[torch.bfloat16]
    assert torch.equal(_bits(xb), _bits(x32.to(torch.bfloat16))) and torch.equal(_bits(mb), _bits(m32.to(torch.bfloat16)))


def test_preprocess_batch_splits_more_than_32_images():
    from codetr import _cabi

    inf = _inferencer()
    images = _images([(20 + i, 30 + 2 * i) for i in range(35)], 12)
    before = _cabi.CALLS["preprocess_batch"]
    x, m, _ = inf.preprocess_batch(images, DEV, torch.float16)
    assert _cabi.CALLS["preprocess_batch"] == before + 2 and x.shape == (35, 3, 768, 1152)
    for i in (0, 31, 32, 34):
        xs, ms, _ = inf.preprocess(images[i], DEV, torch.float16)
        assert torch.equal(_bits(x[i]), _bits(xs[0])) and torch.equal(_bits(m[i]), _bits(ms[0]))


# ---- 2. post-processing -------------------------------------------------------------------------------------------
def _detections(dtype, thr, N=4, Q=300, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(N, Q, 2, generator=g) * 800
    wh = torch.rand(N, Q, 2, generator=g) * 150 + 2
    boxes = torch.cat((c, c + wh), -1)
    boxes[:, Q // 2:] = boxes[:, :Q - Q // 2] + (torch.rand(N, Q - Q // 2, 4, generator=g) - 0.5) * 6  # near duplicates
    boxes[:, 7:12, 2] = boxes[:, 7:12, 0]                       # zero-area boxes
    boxes[:, 12:14] = boxes[:, 7:9]                             # ... and their duplicates
    scores = torch.rand(N, Q, generator=g)
    scores[:, ::17] = scores[:, :1]                             # ties
    scores[:, 3::29] = scores[:, 1:2]
    scores[0, 5] = scores[1, 7] = scores[1, 200] = scores[2, 0] = float("nan")
    scores[3, 9] = scores[0, 150] = -float("nan")                # (sign bit set: sorts last, see codetr_hip.h)
    labels = torch.randint(0, 80, (N, Q), generator=g)          # many classes
    labels[1] = torch.randint(0, 3, (Q,), generator=g)           # few classes: heavy suppression
    labels[3] = 7
    boxes, scores = boxes.to(dtype), scores.to(dtype)
    if thr > 0:
        # scores equal to the threshold rounded to the dtype, and one ulp of the dtype either side of it
        t = torch.tensor(thr, dtype=torch.float64).to(dtype).reshape(1)
        tb = t.view(_BITS[dtype])
        near = [t, (tb + 1).view(dtype), (tb - 1).view(dtype)]
        for i, v in enumerate(near * 2):
            scores[i % N, 40 + i] = v[0]
            scores[(i + 1) % N, 60 + i] = v[0]
    return boxes.to(DEV), scores.to(DEV), labels.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("thr,with_nms", [(0.0, True), (0.3, True), (0.3, False), (0.0, False), (0.7, True)])
def test_postprocess_detections_matches_the_per_image_path(dtype, thr, with_nms):
    from codetr import _cabi, hip_ops

    inf = _inferencer(score_threshold=thr, with_nms=with_nms, iou_threshold=0.5)
    boxes, scores, labels = _detections(dtype, thr, seed=int(thr * 10) + 3 * with_nms)
    N = scores.shape[0]
    metas = [dict(scale_factor=sf) for sf in ((0.6, 0.6), (1152 / 1919, 768 / 1281), (1.7, 2.3), (0.25, 0.3333333))]
    before = dict(_cabi.CALLS)
    got = inf.postprocess_batch((boxes, scores, labels), metas)
    assert _cabi.CALLS["postprocess_detections"] == before["postprocess_detections"] + 1
    div = torch.tensor([[m["scale_factor"][0], m["scale_factor"][1]] * 2 for m in metas], dtype=dtype, device=DEV)
    dets = hip_ops.detections_to_host(hip_ops.postprocess_detections(boxes, scores, labels, div, thr if thr > 0 else None,
                                                                     0.5 if with_nms else None))
    for i in range(N):
        (b, s, l), = inf.postprocess_predictions(boxes[i:i + 1], scores[i:i + 1], labels[i:i + 1])
        sf = metas[i]["scale_factor"]
        b = b / b.new_tensor([sf[0], sf[1], sf[0], sf[1]])
        c = int(dets.count[i])
        assert c == l.numel()
        assert torch.equal(dets.labels[i, :c], l.cpu())
        assert torch.equal(_bits(dets.scores[i, :c]), _bits(s)) and torch.equal(_bits(dets.boxes[i, :c]), _bits(b))
        assert bool((dets.labels[i, c:] == 0).all()) and bool((_bits(dets.scores[i, c:]) == 0).all())
        ref = {"labels": l.tolist(), "scores": s.float().tolist(), "bboxes": b.float().tolist()}
        _same([got[i]], [ref])
    if with_nms or thr > 0:
        assert int(dets.count.sum()) < N * scores.shape[1]   # the case removed something


# ---- 3. stub models -----------------------------------------------------------------------------------------------
def _row_model(seen):
    """detections that depend on each image's own input rows only (row 100 of every channel)"""
    def model(x, m):
        seen.append(tuple(x.shape))
        r = x[:, :, 100, :].float()
        scores = torch.sigmoid(r[:, 0, :300] * 2)
        c = torch.stack((r[:, 1, :300] * 80 + 500, r[:, 2, :300] * 60 + 380), -1)
        wh = torch.stack((r[:, 0, 300:600].abs() * 40 + 20, r[:, 1, 300:600].abs() * 40 + 20), -1)
        boxes = torch.cat((c - wh / 2, c + wh / 2), -1)
        labels = (r[:, 2, 600:900].abs() * 10).long() % 5
        return boxes.to(x.dtype), scores.to(x.dtype), labels
    return model


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_batched_call_equals_per_image_call_with_a_stub_model(dtype):
    from codetr import _cabi

    seen = []
    inf = _inferencer(_row_model(seen), score_threshold=0.3)
    images = _images([(480, 640), (1333, 2000), (37, 53), (768, 1152), (600, 900)], 13)
    ref = inf(images, device=DEV, dtype=dtype)["predictions"]
    assert seen == [(1, 3, 768, 1152)] * 5
    seen.clear()
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=dtype, batch_size=4)["predictions"]
    assert seen == [(4, 3, 768, 1152), (1, 3, 768, 1152)]
    assert _cabi.CALLS["preprocess_batch"] - before["preprocess_batch"] == 2
    assert _cabi.CALLS["postprocess_detections"] - before["postprocess_detections"] == 2
    assert _cabi.CALLS["preprocess"] == before["preprocess"] and _cabi.CALLS["batched_nms"] == before["batched_nms"]
    assert sum(len(p["labels"]) for p in ref) > 10
    _same(got, ref)
    assert inf.num_predicted_imgs == 10


def test_divisor_padded_config_stacks_like_mmdet():
    """R50 config (Resize(1333, 800), no Pad) with pad_size_divisor 32: each image keeps its own resized shape, the batch
    is the largest of them rounded up to 32 (mmdet stack_batch); what each image sees is what it sees alone"""
    from codetr.inferencer import rescale_size

    seen = []
    inf = _inferencer(_row_model(seen), cfg=R50, pad_size_divisor=32, pad_value=0.0)
    assert inf.pad_size is None and inf.scale == (1333, 800)
    sizes = [(480, 640), (1000, 300), (333, 517)]
    images = _images(sizes, 14)
    x, m, metas = inf.preprocess_batch(images, DEV, torch.float32)
    shapes = [rescale_size(h, w, (1333, 800)) for h, w in sizes]
    Hb, Wb = -(-max(s[0] for s in shapes) // 32) * 32, -(-max(s[1] for s in shapes) // 32) * 32
    assert x.shape == (3, 3, Hb, Wb) and [mt["img_shape"] for mt in metas] == shapes
    for i, img in enumerate(images):
        xs, ms, meta = inf.preprocess(img, DEV, torch.float32)
        Hd, Wd = meta["pad_shape"]
        assert metas[i]["pad_shape"] == (Hd, Wd) and Hd % 32 == 0 and Wd % 32 == 0
        assert torch.equal(x[i, :, :Hd, :Wd], xs[0]) and torch.equal(m[i, :Hd, :Wd], ms[0])
        assert float(x[i, :, Hd:, :].abs().sum()) == 0.0 and float(x[i, :, :, Wd:].abs().sum()) == 0.0
        assert bool((m[i, Hd:, :] == 1).all()) and bool((m[i, :, Wd:] == 1).all())
    inf(images, device=DEV, batch_size=3)
    assert seen[-1] == (3, 3, Hb, Wb)


def test_bf16_runs_the_batched_path_at_batch_size_one():
    from codetr import _cabi

    seen = []
    inf = _inferencer(_row_model(seen), score_threshold=0.3)
    images = _images([(480, 640), (600, 900)], 15)
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=torch.bfloat16)["predictions"]
    assert seen == [(1, 3, 768, 1152)] * 2 and len(got) == 2
    assert _cabi.CALLS["preprocess_batch"] - before["preprocess_batch"] == 2
    assert _cabi.CALLS["preprocess"] == before["preprocess"]
    with pytest.raises(ValueError):
        inf(images, device=DEV, batch_size=0)


# ---- 4. tiny real model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_tiny_model_batched_inferencer(dtype):
    import codetr
    from codetr import _cabi
    from helpers_model import seeded_params
    from test_model_gpu import _tiny_codetr_cfg

    torch.manual_seed(0)
    model = codetr.CoDETR(**_tiny_codetr_cfg("swin"))
    spec = [(k, tuple(v.shape)) for k, v in model.named_parameters()]
    full = dict(model.state_dict())
    full.update(seeded_params(spec, 77, scale=1.5))
    model.load_state_dict(full)
    model = model.to(DEV, dtype).eval()
    inf = _inferencer(model)
    images = _images([(480, 640), (1333, 2000), (768, 1152), (300, 1000), (777, 555)], 16)
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=dtype, batch_size=3)["predictions"]
    assert _cabi.CALLS["preprocess_batch"] - before["preprocess_batch"] == 2
    assert _cabi.CALLS["postprocess_detections"] - before["postprocess_detections"] == 2
    assert _cabi.CALLS["preprocess"] == before["preprocess"] and _cabi.CALLS["batched_nms"] == before["batched_nms"]
    assert len(got) == 5
    expect = []
    with torch.no_grad():
        for chunk in (images[:3], images[3:]):
            x, m, metas = inf.preprocess_batch(chunk, DEV, dtype)
            preds = model(x, m)
            batch = inf.postprocess_batch(preds, metas)
            expect += batch
            # ... which is the per-image post-processing of the same forward
            for i, (b, s, l) in enumerate(inf.postprocess_predictions(*preds)):
                sf = metas[i]["scale_factor"]
                b = b / b.new_tensor([sf[0], sf[1], sf[0], sf[1]])
                _same([batch[i]], [{"labels": l.tolist(), "scores": s.float().tolist(), "bboxes": b.float().tolist()}])
    _same(got, expect)
    assert sum(len(p["labels"]) for p in got) > 0
