"""GPU: weighted boxes fusion -- codetr_wbf_merge_* bit for bit against the numpy restatement of its header text
(tests/wbf_ref.py) with guard rows around every output, `hip_ops.weighted_boxes_fusion` on ragged lists, and
`Inferencer(tta=dict(wbf=...), ensemble=[...])` against the composition of its steps."""
import numpy as np
import pytest
import torch

import wbf_ref as R
from test_inferencer_batch_gpu import DEV, SWIN, _bits, _images, _same
from test_tta_gpu import _mirror, _stub, _to_storage

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CONF = ["avg", "max"]
LAYOUTS = ["eighty", "three", "one"]
GUARD = 0x5A


def _scene(dtype, V, N, Q, layout, kind, full, seed):
    """the stacked per-view detections of N images (CPU tensors).  kind 'jitter': every view sees the same Q objects,
    slightly moved; 'same': every candidate is one box; 'disjoint': no two candidates overlap.  Scores hold ties across
    and inside views, +0, -0 and a NaN; the counts are ragged unless `full`, with an empty view and an empty image at N = 3"""
    g = torch.Generator().manual_seed(seed)
    widths = torch.tensor([1000.0, 640.0, 333.0][:N])
    if kind == "same":
        boxes = torch.tensor([100.0, 50.0, 180.0, 90.0]).expand(V, N, Q, 4).clone()
    elif kind == "disjoint":
        i = torch.arange(V * Q, dtype=torch.float32).view(V, 1, Q).expand(V, N, Q)
        x, y = (i % 64) * 8, torch.floor(i / 64) * 8                    # an 8-pixel grid of 6 x 5 boxes: exact in bf16
        boxes = torch.stack((x, y, x + 6, y + 5), -1)
    else:
        c = torch.rand(N, Q, 2, generator=g) * 500
        wh = torch.rand(N, Q, 2, generator=g) * 150 + 8
        base = torch.cat((c, c + wh), -1)
        if Q > 12:
            base[:, 7:10, 2] = base[:, 7:10, 0]                          # (nearly) zero-area boxes, negative widths
            base[:, 10:12] = base[:, 7:9]                                # ... and their duplicates
        boxes = base[None] + (torch.rand(V, N, Q, 4, generator=g) - 0.5) * 6
        if V > 1:
            boxes[1, :, ::5] = boxes[0, :, ::5]                          # exact duplicates across two views
    scores = torch.rand(V, N, Q, generator=g) * 0.95 + 0.05
    if V > 1:
        scores[1:, :, ::3] = scores[:1, :, ::3]                          # ties across views: the lowest c decides
    scores[:, :, 1::7] = scores[:, :, :1]                                # ... and inside a view
    if Q > 4:
        scores[0, :, 2] = -0.0
        scores[V - 1, :, 3] = 0.0
        scores[V - 1, 0, 4] = float("nan")
    if layout == "one":
        labels = torch.full((V, N, Q), 5)
    elif layout == "three":
        labels = torch.randint(0, 3, (N, Q), generator=g)[None].expand(V, N, Q).clone() * 40 - 7   # a negative label too
    else:
        labels = torch.randint(0, 80, (N, Q), generator=g)[None].expand(V, N, Q).clone()
        labels[0, :, ::11] = torch.randint(0, 80, (N, len(range(0, Q, 11))), generator=g)          # views may disagree
    count = torch.full((V, N), Q, dtype=torch.int32)
    if not full:
        count[:, 0] = torch.randint(0, Q + 1, (V,), generator=g).to(torch.int32)                   # ragged
    if N == 3:
        count[:, 1] = torch.randint(1, Q + 1, (V,), generator=g).to(torch.int32)
        count[V // 2, 1] = 0                                                                        # a view with nothing
        count[:, 2] = 0                                                                             # an image with nothing
    return boxes.to(dtype), scores.to(dtype), labels, count, widths


def _guarded(shape, dtype):
    """an output with one guard row of GUARD bytes before and after its N rows -> (whole, the N rows)"""
    whole = torch.empty((shape[0] + 2,) + tuple(shape[1:]), dtype=dtype, device=DEV)
    whole.view(torch.uint8).fill_(GUARD)
    return whole, whole[1:-1]


def _fuse_and_compare(dtype, conf_type, V, N, Q, layout, kind, flips, full, seed, weights=None, skip=0.0, keep=None,
                      iou=0.55):
    """one launch on outputs with guard rows, every field against the reference -> (candidates, clusters, most votes)"""
    from codetr import _cabi, _wbf

    boxes, scores, labels, count, widths = _scene(dtype, V, N, Q, layout, kind, full, seed)
    boxes = _mirror(boxes, flips, widths)
    K = keep if keep else V * Q
    outs = [_guarded((N, K, 4), dtype), _guarded((N, K), dtype), _guarded((N, K), torch.int64),
            _guarded((N, K), torch.int32), _guarded((N,), torch.int32), _guarded((N, K), torch.int32)]
    before = _cabi.CALLS["wbf_merge"]
    _wbf.wbf_merge(boxes.to(DEV), scores.to(DEV), labels.to(DEV), count.to(DEV), sum(1 << v for v, f in enumerate(flips) if f),
                   widths.to(DEV), weights, _wbf.CONF_TYPES[conf_type], iou, skip, keep or 0, *[o[1] for o in outs])
    assert _cabi.CALLS["wbf_merge"] == before + 1
    torch.cuda.synchronize()
    for whole, _ in outs:                                      # the guard rows are untouched
        raw = whole.view(whole.shape[0], -1).view(torch.uint8).cpu()
        assert bool((raw[0] == GUARD).all()) and bool((raw[-1] == GUARD).all())
    gb, gs, gl, gi, gc, gv = (o[1].cpu() for o in outs)
    ts = _to_storage(dtype)
    cand = clusters = most = 0
    for n in range(N):
        eb, es, el, ei, ev = R.fuse_outputs(boxes[:, n].float().numpy(), scores[:, n].float().numpy(), labels[:, n].numpy(),
                                            count[:, n].numpy(), flips, float(widths[n]), ts, weights=weights,
                                            conf_type=conf_type, iou_threshold=iou, skip_box_thr=skip, max_keep=keep or 0)
        c = int(gc[n])
        print(f"{dtype} {conf_type} V={V} Q={Q} {layout} {kind} n={n}: candidates {int(count[:, n].sum())} -> {c} clusters, "
              f"most votes {int(ev.max()) if len(ev) else 0}")
        assert c == len(ei)
        assert gi[n, :c].tolist() == ei.tolist()
        assert gv[n, :c].tolist() == ev.tolist()
        assert gl[n, :c].tolist() == el.tolist()
        assert torch.equal(_bits(gb[n, :c]), _bits(eb))
        assert torch.equal(_bits(gs[n, :c]), _bits(es))
        assert bool((gl[n, c:] == 0).all()) and bool((gi[n, c:] == 0).all()) and bool((gv[n, c:] == 0).all())
        assert bool((_bits(gs[n, c:]) == 0).all()) and bool((_bits(gb[n, c:]) == 0).all())
        cand += int(count[:, n].sum())
        clusters += c
        most = max(most, int(ev.max()) if len(ev) else 0)
    return cand, clusters, most


VQ = [(1, 1), (2, 8), (3, 64), (6, 300), (16, 256)]


@pytest.mark.parametrize("V,Q", VQ)
@pytest.mark.parametrize("conf_type", CONF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wbf_merge_matches_the_reference(dtype, conf_type, V, Q):
    """N, the label layout, the counts, the flip mask and the weights rotate with the case; (16, 256) is the limit of
    4096 candidates: every slot a candidate, and once per conf_type (in f32) all of them in one chain"""
    case = VQ.index((V, Q)) + DTYPES.index(dtype) + CONF.index(conf_type)
    layout = LAYOUTS[case % 3]
    N, full = (3 if case % 2 == 0 else 1), case % 3 == 1
    if (V, Q) == (16, 256):
        N, full = 1, True
        layout = "one" if dtype == torch.float32 else "eighty"
    flips = [(v + case) % 3 == 0 for v in range(V)]
    weights = None if case % 2 else [1.0 + 0.25 * ((v * 5 + case) % 4) for v in range(V)]
    cand, clusters, most = _fuse_and_compare(dtype, conf_type, V, N, Q, layout, "jitter", flips, full, seed=10 * case + V,
                                             weights=weights)
    if V > 1 and cand >= 10:
        assert clusters < cand and most >= 2                    # the views' near duplicates did fuse


@pytest.mark.parametrize("kind", ["jitter", "same", "disjoint"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_label_and_box_layouts(layout, kind):
    V, N, Q = 3, 3, 64
    cand, clusters, most = _fuse_and_compare(torch.float16, "avg", V, N, Q, layout, kind, [False, True, False], False,
                                             seed=40 + LAYOUTS.index(layout))
    if kind == "same" and layout == "one":
        assert clusters == 2 and most > V                       # one cluster per non-empty image, more votes than views
    if kind == "disjoint":
        assert most == 1                                        # every live candidate is its own cluster
    # the 64-bit masks (more than 1024 slots) on the same layouts
    _fuse_and_compare(torch.float32, "max", 5, 1, 300, layout, kind, [False] * 5, True, seed=50)


def test_every_flip_mask_at_three_views():
    for mask in range(8):
        for N in (1, 3):
            _fuse_and_compare(torch.float16, "avg", 3, N, 40, "three", "jitter", [bool(mask >> v & 1) for v in range(3)],
                              N == 1, seed=60 + mask)


def test_weights_skip_threshold_and_the_cut():
    args = (torch.float32, "avg", 4, 3, 50, "eighty", "jitter", [False, True, False, True], True)
    cand, clusters, _ = _fuse_and_compare(*args, seed=70, weights=[2.0, 1.0, 0.5, 1.5])
    assert _fuse_and_compare(*args, seed=70, skip=0.3)[1] < clusters        # candidates under 0.3 never found a cluster
    _fuse_and_compare(torch.bfloat16, "max", 4, 3, 50, "eighty", "jitter", [False] * 4, True, seed=71,
                      weights=[2.0, 1.0, 0.5, 1.5], skip=0.3)
    for keep in (1, 17, 5000):          # below the cluster count; 5000 > V * Q: K follows max_keep, the rest is zero
        assert _fuse_and_compare(*args, seed=70, keep=keep)[1] <= 3 * keep
    _fuse_and_compare(*args, seed=72, iou=0.3)
    _fuse_and_compare(*args, seed=72, iou=0.9)


def _lists(rows, V):
    per = [[r for r in rows if r[0] == v] for v in range(V)]
    return ([[r[1] for r in p] for p in per], [[r[2] for r in p] for p in per], [[r[3] for r in p] for p in per])


def test_tie_and_drop_rules_through_weighted_boxes_fusion():
    from codetr import hip_ops

    # equal overlaps (80 / 120 with both founders): the lower founder c, not the first-created cluster
    rows = [(0, (0, 0, 10, 10), 0.5, 3), (0, (4, 0, 14, 10), 0.75, 3), (1, (2, 0, 12, 10), 0.375, 3)]
    bx, sc, lab = hip_ops.weighted_boxes_fusion(*_lists(rows, 2))
    assert sc.tolist() == [0.4375, 0.375] and lab.tolist() == [3, 3]
    assert bx.tolist() == [[float(np.float32(0.75) / np.float32(0.875)), 0.0, float(np.float32(9.5) / np.float32(0.875)), 10.0],
                           [4.0, 0.0, 14.0, 10.0]]
    # the two known answers of the header's rule
    bx, sc, lab = hip_ops.weighted_boxes_fusion(*_lists([(0, (0, 0, 10, 10), 0.9, 7), (1, (1, 1, 11, 11), 0.6, 7)], 2))
    assert sc.tolist() == [0.75] and bx[0].tolist() == [float(np.float32(v)) for v in (0.4, 0.4, 10.400001, 10.400001)]
    bx, sc, lab = hip_ops.weighted_boxes_fusion(*_lists([(0, (50, 50, 60, 60), 0.8, 1)], 2))
    assert sc.tolist() == [float(np.float32(0.4))] and bx.tolist() == [[50.0, 50.0, 60.0, 60.0]]
    # zero and NaN scores are dropped; an IoU equal to the threshold does not join
    rows = [(0, (0, 0, 10, 10), 0.0, 1), (0, (0, 0, 10, 10), float("nan"), 1), (1, (0, 0, 10, 10), 0.5, 1)]
    bx, sc, lab = hip_ops.weighted_boxes_fusion(*_lists(rows, 2))
    assert sc.tolist() == [0.25]
    rows = [(0, (0, 0, 2, 2), 0.5, 1), (1, (0, 0, 2, 1), 0.25, 1)]
    assert len(hip_ops.weighted_boxes_fusion(*_lists(rows, 2), iou_thr=0.5)[1]) == 2
    assert len(hip_ops.weighted_boxes_fusion(*_lists(rows, 2), iou_thr=0.49)[1]) == 1
    # max with weights [2, 1]
    rows = [(0, (0, 0, 10, 10), 0.5, 2), (1, (0, 0, 10, 10), 0.9, 2), (1, (50, 50, 60, 60), 0.4, 2)]
    bx, sc, lab = hip_ops.weighted_boxes_fusion(*_lists(rows, 2), weights=[2, 1], conf_type="max")
    assert sc.tolist() == [0.5, float(np.float32(0.4) / np.float32(2))]


def test_weighted_boxes_fusion_on_ragged_lists_equals_the_reference():
    from codetr import _cabi, hip_ops

    rng = np.random.default_rng(5)
    lengths = [5, 0, 17, 3]
    truth = rng.uniform(0, 1, (17, 2)) * 0.7                          # normalised coordinates
    obj = np.concatenate([truth, truth + rng.uniform(0.05, 0.3, (17, 2))], 1)
    boxes_list = [np.abs(obj[:n] + rng.normal(0, 0.004, (n, 4))).astype(np.float32) for n in lengths]
    scores_list = [rng.uniform(0.05, 1, n).astype(np.float32) for n in lengths]
    labels_list = [np.arange(n) % 2 for n in lengths]
    weights = [1.0, 3.0, 2.0, 0.5]
    before = _cabi.CALLS["wbf_merge"]
    bx, sc, lab = hip_ops.weighted_boxes_fusion(boxes_list, [torch.from_numpy(s).to(DEV) for s in scores_list], labels_list,
                                                weights=weights, iou_thr=0.5, skip_box_thr=0.1, conf_type="avg")
    assert _cabi.CALLS["wbf_merge"] == before + 1 and bx.is_cuda and bx.dtype == sc.dtype == torch.float32
    V, Q = 4, 17
    b, s, l = np.zeros((V, Q, 4), np.float32), np.zeros((V, Q), np.float32), np.zeros((V, Q), np.int64)
    for v, n in enumerate(lengths):
        b[v, :n], s[v, :n], l[v, :n] = boxes_list[v], scores_list[v], labels_list[v]
    eb, es, el, _, ev = R.fuse(b, s, l, lengths, [False] * V, 0.0, weights=weights, iou_threshold=0.5, skip_box_thr=0.1)
    assert len(es) > 5 and ev.max() >= 2
    assert np.array_equal(bx.cpu().numpy(), eb) and np.array_equal(sc.cpu().numpy(), es) and lab.tolist() == el.tolist()
    empty = hip_ops.weighted_boxes_fusion([np.zeros((0, 4))], [np.zeros(0)], [np.zeros(0)])
    assert [tuple(t.shape) for t in empty] == [(0, 4), (0,), (0,)]
    with pytest.raises(ValueError):
        hip_ops.weighted_boxes_fusion(boxes_list, scores_list[:3], labels_list)
    with pytest.raises(ValueError):
        hip_ops.weighted_boxes_fusion(boxes_list, scores_list, labels_list, weights=[1, 2])
    with pytest.raises(NotImplementedError):
        hip_ops.weighted_boxes_fusion(boxes_list, scores_list, labels_list, conf_type="box_and_model_avg")


def test_host_side_limits_launch_nothing():
    from codetr import _cabi, _wbf, hip_ops
    from test_wbf_cpu import reject_cases

    _cabi.RECORDER = []
    try:
        before = _cabi.CALLS["wbf_merge"]
        for suffix in ("f16", "bf16", "f32"):
            for what, got, want in reject_cases(getattr(_wbf.load(), "codetr_wbf_merge_" + suffix)):
                assert got == want, (suffix, what)
        assert _cabi.RECORDER == [] and _cabi.CALLS["wbf_merge"] == before
    finally:
        _cabi.RECORDER = None

    def dets(rows, Q):
        return hip_ops.Detections(torch.zeros((rows, Q, 4), device=DEV), torch.zeros((rows, Q), device=DEV),
                                  torch.zeros((rows, Q), dtype=torch.int64, device=DEV),
                                  torch.zeros((rows,), dtype=torch.int32, device=DEV), None)

    with pytest.raises(ValueError, match="4096"):
        hip_ops.wbf_merge([dets(1, 1025)] * 5, [False] * 5, [10.0])
    with pytest.raises(ValueError, match="16"):
        hip_ops.wbf_merge([dets(17, 2)], [False] * 17, [10.0])
    with pytest.raises(ValueError):
        hip_ops.wbf_merge([dets(2, 5)], [False], [10.0])                      # two views, one flag
    with pytest.raises(ValueError, match="weights"):
        hip_ops.wbf_merge([dets(2, 5)], [False, True], [10.0], dict(weights=[1, 2, 3]))
    with pytest.raises(ValueError):
        hip_ops.wbf_merge([dets(2, 5)], [False, True], [10.0], dict(iou_thr=0.5))
    assert _cabi.CALLS["wbf_merge"] == before
    out = hip_ops.detections_to_host(hip_ops.wbf_merge([dets(2, 5)], [False, True], [10.0]))
    assert isinstance(out, hip_ops.WbfDetections) and int(out.count[0]) == 0   # counts of zero: nothing to fuse
    assert out.scores.shape == out.votes.shape == (1, 10) and out.votes.dtype == torch.int32


# ---- the Inferencer -------------------------------------------------------------------------------------------------
TTA = dict(scales=[(320, 200), (400, 256)], flip=True)


def _stub_b(seen, Q=64):
    """a second model: the first one's detections moved and less sure of themselves"""
    base = _stub(seen, Q)

    def model(x, m):
        boxes, scores, labels = base(x, m)
        return (boxes.float() + 3).to(x.dtype), (scores.float() * 0.875).to(x.dtype), labels
    return model


def _composed(inf, models, images, dtype, batch_size, weights):
    """the call restated without the Inferencer's TTA methods: the row table from rescale_size, hip_ops.preprocess_views,
    every model on the same views, postprocess_device, and wbf_ref per image over the views in the stated order
    v = (k * S + s) * F + f with the per-view `weights` written out by the caller"""
    from codetr import hip_ops
    from codetr.inferencer import rescale_size

    t, out = inf.tta, []
    flips = (False, True) if t["flip"] else (False,)
    ts = _to_storage(dtype)
    d = inf.pad_size_divisor
    for start in range(0, len(images), batch_size):
        chunk = images[start:start + batch_size]
        N = len(chunk)
        src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in chunk])).to(DEV)
        offsets = np.cumsum([0] + [im.size for im in chunk]).tolist()
        per_model = [[] for _ in models]
        for scale in t["scales"]:
            rows, metas = [], []
            for f in flips:                                   # flip-major: row f * N + n
                for o, im in zip(offsets, chunk):
                    H, W = im.shape[:2]
                    nh, nw = rescale_size(H, W, scale)
                    rows.append((o, H, W, nh, nw, nh, nw, int(f)))
                    metas.append(dict(scale_factor=(nw / W, nh / H)))
            Hb = max(-(-r[3] // d) * d for r in rows)
            Wb = max(-(-r[4] // d) * d for r in rows)
            x, m = hip_ops.preprocess_views(src, rows, (Hb, Wb), inf.mean, inf.std, inf.pad_val, inf.pad_value, dtype)
            for k, model in enumerate(models):
                with torch.no_grad():
                    h = hip_ops.detections_to_host(inf.postprocess_device(model(x, m), metas))
                Q = h.scores.shape[1]
                per_model[k].append((h.boxes.view(len(flips), N, Q, 4), h.scores.view(len(flips), N, Q),
                                     h.labels.view(len(flips), N, Q), h.count.view(len(flips), N)))
        views = [v for per in per_model for v in per]
        b, s, l, c = (torch.cat([v[i] for v in views]) for i in range(4))
        view_flips = [f for _ in models for _ in t["scales"] for f in flips]
        for n, im in enumerate(chunk):
            eb, es, el, _, ev = R.fuse_outputs(b[:, n].float().numpy(), s[:, n].float().numpy(), l[:, n].numpy(),
                                               c[:, n].numpy(), view_flips, float(im.shape[1]), ts, weights=weights,
                                               conf_type=t["wbf"]["conf_type"], iou_threshold=t["wbf"]["iou_threshold"],
                                               skip_box_thr=t["wbf"]["skip_box_thr"], max_keep=t["max_per_img"] or 0)
            out.append({"labels": el.tolist(), "scores": es.float().tolist(), "bboxes": eb.float().tolist(),
                        "votes": ev.tolist()})
    return out


@pytest.mark.parametrize("dtype,wbf", [(torch.float32, dict()), (torch.float16, dict(conf_type="max", iou_threshold=0.5)),
                                       (torch.bfloat16, dict(skip_box_thr=0.4, weights=[1, 2, 1, 0.5]))])
def test_wbf_inferencer_equals_the_composition_with_a_stub_model(dtype, wbf):
    from codetr import _cabi
    from codetr.inferencer import Inferencer

    seen = []
    model = _stub(seen)
    inf = Inferencer(model, SWIN, dataset_meta=None, tta=dict(TTA, wbf=wbf, max_per_img=50), score_threshold=0.3)
    inf.pad_size_divisor, inf.pad_value = 32, 0.5
    images = _images([(480, 640), (1333, 2000), (37, 53), (768, 1152), (600, 900)], 23)
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=dtype, batch_size=2)["predictions"]
    assert _cabi.CALLS["wbf_merge"] - before["wbf_merge"] == 3 and _cabi.CALLS["tta_merge"] == before["tta_merge"]
    assert _cabi.CALLS["preprocess_views"] - before["preprocess_views"] == 3 * 2
    assert [s[0] for s in seen] == [4, 4, 4, 4, 2, 2]
    expect = _composed(inf, [model], images, dtype, 2, wbf.get("weights"))
    _same(got, expect)
    assert [p["votes"] for p in got] == [p["votes"] for p in expect]
    assert all(len(p["votes"]) == len(p["labels"]) <= 50 for p in got)
    assert sum(len(p["labels"]) for p in got) > 10 and max(max(p["votes"]) for p in got if p["votes"]) >= 2
    # the same TTA merged by NMS: no votes, the WBF entry point is not called
    plain = Inferencer(model, SWIN, dataset_meta=None, tta=dict(TTA, max_per_img=50), score_threshold=0.3)
    before = dict(_cabi.CALLS)
    preds = plain(images, device=DEV, dtype=dtype, batch_size=2)["predictions"]
    assert _cabi.CALLS["wbf_merge"] == before["wbf_merge"] and _cabi.CALLS["tta_merge"] == before["tta_merge"] + 3
    assert all("votes" not in p for p in preds)


@pytest.mark.parametrize("merge", ["wbf", "nms"])
def test_ensemble_views_follow_the_stated_order(merge):
    from codetr import _cabi, hip_ops
    from codetr.inferencer import Inferencer
    import tta_ref

    dtype = torch.float16
    seen_a, seen_b = [], []
    a, b = _stub(seen_a), _stub_b(seen_b)
    images = _images([(480, 640), (333, 517), (600, 900)], 29)
    if merge == "wbf":
        tta = dict(TTA, wbf=dict(weights=[2, 1]), max_per_img=60)          # one weight per model
        inf = Inferencer(a, SWIN, dataset_meta=None, tta=tta, score_threshold=0.3, ensemble=[b])
        before = _cabi.CALLS["wbf_merge"]
        got = inf(images, device=DEV, dtype=dtype, batch_size=2)["predictions"]
        assert _cabi.CALLS["wbf_merge"] == before + 2
        assert seen_a == seen_b and [s[0] for s in seen_a] == [4, 4, 2, 2]  # both models on every pre-processed view
        per_view = [2.0] * 4 + [1.0] * 4                                    # v = (k * S + s) * F + f, S = F = 2
        expect = _composed(inf, [a, b], images, dtype, 2, per_view)
        _same(got, expect)
        assert [p["votes"] for p in got] == [p["votes"] for p in expect]
        assert max(max(p["votes"]) for p in got) > 4                        # clusters across both models' views
        wrong = _composed(inf, [b, a], images, dtype, 2, per_view)          # the other order is another answer
        assert any(p["scores"] != q["scores"] for p, q in zip(got, wrong))
        unit = _composed(inf, [a, b], images, dtype, 2, None)               # ... and so are unit weights
        assert any(p["scores"] != q["scores"] for p, q in zip(got, unit))
        with pytest.raises(ValueError, match="one Q"):
            Inferencer(a, SWIN, dataset_meta=None, tta=tta, ensemble=[_stub([], Q=32)])(images[:1], device=DEV, dtype=dtype)
        return
    # an ensemble merged by hard NMS: index names the view in the same order
    inf = Inferencer(a, SWIN, dataset_meta=None, tta=dict(scales=[(320, 200)], flip=True, max_per_img=60),
                     score_threshold=0.3, ensemble=[b])
    got = inf(images, device=DEV, dtype=dtype, batch_size=3)["predictions"]
    rows, metas, hw = inf.view_rows(np.cumsum([0] + [im.size for im in images[:-1]]).tolist(),
                                    [im.shape[:2] for im in images], (320, 200), (False, True))
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    x, m = hip_ops.preprocess_views(src, rows, hw, inf.mean, inf.std, inf.pad_val, inf.pad_value, dtype)
    views = [hip_ops.detections_to_host(inf.postprocess_device(model(x, m), metas)) for model in (a, b)]
    N, Q = 3, views[0].scores.shape[1]
    bx, sc, lb, ct = (torch.cat([getattr(v, f).view(2, N, *getattr(v, f).shape[1:]) for v in views])
                      for f in ("boxes", "scores", "labels", "count"))
    for n, im in enumerate(images):
        eb, es, el, _ = tta_ref.merge_outputs(bx[:, n].float().numpy(), sc[:, n].float().numpy(), lb[:, n].numpy(),
                                              ct[:, n].numpy(), [False, True] * 2, float(im.shape[1]), _to_storage(dtype),
                                              "nms", 0.5, 1e-3, 60)
        _same([got[n]], [{"labels": el.tolist(), "scores": es.float().tolist(), "bboxes": eb.float().tolist()}])


def test_wbf_predictions_feed_the_drawing():
    from codetr import _cabi
    from codetr.inferencer import Inferencer
    import draw_ref

    names = ["person", "bicycle", "car"]
    images = _images([(480, 640), (333, 517), (600, 900)], 31)
    inf = Inferencer(_stub([]), SWIN, None, score_threshold=0.3, visualizer=dict(classes=names, line_width=2, alpha=0.6),
                     tta=dict(scales=[(320, 200)], flip=True, wbf={}, max_per_img=50))
    before = _cabi.CALLS["draw_detections"]
    out = inf(images, return_vis=True, pred_score_thr=0.2, device=DEV, dtype=torch.float16, batch_size=2)
    assert _cabi.CALLS["draw_detections"] == before + 2 and len(out["visualization"]) == 3
    font, total = _cabi.draw_font(), 0
    for img, pred, drawn in zip(images, out["predictions"], out["visualization"]):
        assert "votes" in pred
        ref = draw_ref.draw(img, np.asarray(pred["bboxes"], np.float32).reshape(-1, 4), np.asarray(pred["scores"], np.float32),
                            pred["labels"], names, inf.visualizer["palette"], font, dict(line_width=2, alpha=0.6, score_thr=0.2))
        assert np.array_equal(drawn, ref)
        total += int((drawn != img).any(-1).sum())
    assert total > 1000
