"""GPU: test-time augmentation in the Inferencer -- codetr_preprocess_views_u8_* against preprocess_batch and its own
mirror image, codetr_tta_merge_* bit for bit against the numpy restatement of its header text (tests/tta_ref.py), and
`Inferencer(tta=...)` against the composition of its four steps."""
import numpy as np
import pytest
import torch

import tta_ref as R
from test_inferencer_batch_gpu import DEV, SWIN, _bits, _images, _same

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MODES = ["nms", "naive", "linear"]


def _to_storage(dtype):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)


# ---- 1. preprocessing of views ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_preprocess_views_mirrors_inside_the_resized_width(dtype):
    from codetr import _cabi, hip_ops
    from codetr.inferencer import rescale_size

    sizes = [(1, 1), (37, 53), (333, 517), (100, 1500)]
    images = _images(sizes, 21)
    mean, std, pad_val, fill = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375), (114, 7, 250), 0.5
    rows7, rows8, off = [], [], 0
    for (h, w) in sizes:
        nh, nw = rescale_size(h, w, (400, 256))
        row = (off, h, w, nh, nw, nh + 3, nw + 7)        # a Pad region beyond the image, then the divisor padding
        rows7.append(row)
        rows8 += [row + (0,), row + (1,)]                 # both views read the one uploaded image
        off += h * w * 3
    widths = [r[4] for r in rows7]
    assert max(widths) > 256 and any(w % 2 for w in widths) and widths == [256, 367, 397, 400]
    Hb, Wb = 288, 416
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    before = dict(_cabi.CALLS)
    x, m = hip_ops.preprocess_views(src, rows8, (Hb, Wb), mean, std, pad_val, fill, dtype)
    assert _cabi.CALLS["preprocess_views"] == before["preprocess_views"] + 1
    assert _cabi.CALLS["preprocess_batch"] == before["preprocess_batch"]
    xr, mr = hip_ops.preprocess_batch(src, rows7, (Hb, Wb), mean, std, pad_val, fill, dtype)
    assert x.shape == (8, 3, Hb, Wb) and m.shape == (8, Hb, Wb) and x.dtype == m.dtype == dtype
    # unflipped rows: the batch kernel's result, bit for bit
    assert torch.equal(_bits(x[0::2]), _bits(xr)) and torch.equal(_bits(m[0::2]), _bits(mr))
    for i, row in enumerate(rows7):
        nh, nw = row[3], row[4]
        plain, flipped = x[2 * i], x[2 * i + 1].clone()
        # inside the resized image: the mirror image; everything outside it, and the mask, as unflipped
        assert torch.equal(_bits(flipped[:, :nh, :nw]), _bits(plain[:, :nh, :nw].flip(-1)))
        flipped[:, :nh, :nw] = plain[:, :nh, :nw]
        assert torch.equal(_bits(flipped), _bits(plain))
        assert torch.equal(_bits(m[2 * i + 1]), _bits(m[2 * i]))
        if row[2] > 1:    # (a one-pixel source resizes to a constant image)
            assert not torch.equal(_bits(x[2 * i + 1, :, :nh, :nw]), _bits(plain[:, :nh, :nw]))   # it did mirror


def test_preprocess_views_splits_more_than_32_rows():
    from codetr import _cabi, hip_ops

    img = _images([(20, 30)], 22)[0]
    src = torch.from_numpy(img.reshape(-1)).to(DEV)
    rows = [(0, 20, 30, 40, 60, 40, 60, i % 2) for i in range(35)]
    before = _cabi.CALLS["preprocess_views"]
    x, _ = hip_ops.preprocess_views(src, rows, (64, 64), (0, 0, 0), (1, 1, 1), dtype=torch.float16)
    assert _cabi.CALLS["preprocess_views"] == before + 2
    assert torch.equal(_bits(x[34]), _bits(x[0])) and torch.equal(_bits(x[33]), _bits(x[1]))
    assert torch.equal(_bits(x[1, :, :40, :60]), _bits(x[0, :, :40, :60].flip(-1)))
    with pytest.raises(ValueError):
        hip_ops.preprocess_views(src, [r[:7] for r in rows], (64, 64), (0, 0, 0), (1, 1, 1))


# ---- 2. the merge -------------------------------------------------------------------------------------------------
LAYOUTS = ["one", "two", "eighty", "own"]
FLIPS = ["none", "all", "alternating"]


def _flip_list(kind, V):
    return [kind == "all" or (kind == "alternating" and v % 2 == 1) for v in range(V)]


def _views(dtype, V, N, Q, layout, full, seed):
    """the stacked per-view detections of N images (CPU tensors): every view sees the same Q objects, slightly moved
    (near duplicates across views: NMS has work), stored mirrored where the view is flipped"""
    g = torch.Generator().manual_seed(seed)
    widths = torch.tensor([1000.0, 640.0, 333.0][:N])
    c = torch.rand(N, Q, 2, generator=g) * 500
    wh = torch.rand(N, Q, 2, generator=g) * 150 + 2
    base = torch.cat((c, c + wh), -1)
    if Q > 12:
        base[:, 7:10, 2] = base[:, 7:10, 0]                       # zero-area boxes
        base[:, 10:12] = base[:, 7:9]                             # ... and their duplicates
    boxes = base[None] + (torch.rand(V, N, Q, 4, generator=g) - 0.5) * 6
    if V > 1:
        boxes[1, :, ::5] = boxes[0, :, ::5]                       # exact duplicates across two views
    scores = torch.rand(V, N, Q, generator=g)
    if V > 1:
        scores[1:, :, ::3] = scores[:1, :, ::3]                   # ties across views: the lowest c decides
    scores[:, :, 1::7] = scores[:, :, :1]                         # ... and inside a view
    if Q > 4:
        scores[0, :, 2] = -0.0
        scores[V - 1, :, 3] = 0.0
        scores[V - 1, 0, 4] = float("nan")
    if layout == "one":
        labels = torch.full((V, N, Q), 5)
    elif layout == "two":
        labels = torch.randint(0, 2, (N, Q), generator=g)[None].expand(V, N, Q).clone() * 40 + 3
    elif layout == "eighty":
        labels = torch.randint(0, 80, (N, Q), generator=g)[None].expand(V, N, Q).clone()
        labels[0, :, ::11] = torch.randint(0, 80, (N, len(range(0, Q, 11))), generator=g)   # views may disagree
    else:
        labels = torch.arange(V * Q).view(V, 1, Q).expand(V, N, Q).clone() * 3 - 100        # negative labels too
    count = torch.full((V, N), Q, dtype=torch.int32)
    if not full:
        count[:, 0] = torch.randint(0, Q + 1, (V,), generator=g).to(torch.int32)           # ragged
    if N == 3:
        count[:, 1] = torch.randint(1, Q + 1, (V,), generator=g).to(torch.int32)
        count[V // 2, 1] = 0                                                                # a view with nothing
        count[:, 2] = 0                                                                     # an image with nothing
    return boxes.to(dtype), scores.to(dtype), labels, count, widths


def _mirror(boxes, flips, widths):
    """store the flipped views' boxes as those views report them: mirrored in the image (exactly, in the dtype)"""
    out = boxes.clone()
    W = widths.view(1, -1, 1).to(boxes.dtype)
    for v, f in enumerate(flips):
        if f:
            out[v, ..., 0] = W[0] - boxes[v, ..., 2]
            out[v, ..., 2] = W[0] - boxes[v, ..., 0]
    return out


def _merge_and_compare(dtype, mode, V, N, Q, layout, flip_kind, full, seed, max_per_img=None, iou=0.5):
    """-> (candidates, emitted, decayed) summed over the images"""
    from codetr import _cabi, hip_ops

    flips = _flip_list(flip_kind, V)
    boxes, scores, labels, count, widths = _views(dtype, V, N, Q, layout, full, seed)
    boxes = _mirror(boxes, flips, widths)
    nms = dict(type="nms", iou_threshold=iou) if mode == "nms" else dict(type="soft_nms", iou_threshold=iou, method=mode,
                                                                         min_score=0.05)
    # one entry per view, as the Inferencer passes them; the packed buffer is unused by the merge
    dets = [hip_ops.Detections(boxes[v].to(DEV), scores[v].to(DEV), labels[v].to(DEV), count[v].to(DEV), None)
            for v in range(V)]
    before = _cabi.CALLS["tta_merge"]
    out = hip_ops.tta_merge(dets, flips, widths.to(DEV), nms, max_per_img)
    assert _cabi.CALLS["tta_merge"] == before + 1
    host = hip_ops.detections_to_host(out)
    K = max_per_img if max_per_img else V * Q
    assert host.scores.shape == (N, K) and host.boxes.shape == (N, K, 4) and host.index.shape == (N, K)
    ts = _to_storage(dtype)
    cand = emitted = decayed = 0
    for n in range(N):
        eb, es, el, ei = R.merge_outputs(boxes[:, n].float().numpy(), scores[:, n].float().numpy(), labels[:, n].numpy(),
                                         count[:, n].numpy(), flips, float(widths[n]), ts, mode, iou, 0.05,
                                         max_per_img or 0)
        c = int(host.count[n])
        print(f"{dtype} {mode} V={V} Q={Q} {layout} {flip_kind} n={n}: candidates {int(count[:, n].sum())} -> {c}")
        assert c == len(ei)
        assert host.index[n, :c].tolist() == ei.tolist()
        assert host.labels[n, :c].tolist() == el.tolist()
        assert torch.equal(_bits(host.boxes[n, :c]), _bits(eb))
        gs, nan = host.scores[n, :c], torch.isnan(es)
        assert torch.equal(torch.isnan(gs), nan) and torch.equal(_bits(gs[~nan]), _bits(es[~nan]))
        assert bool((host.labels[n, c:] == 0).all()) and bool((host.index[n, c:] == 0).all())
        assert bool((_bits(host.scores[n, c:]) == 0).all()) and bool((_bits(host.boxes[n, c:]) == 0).all())
        cand += int(count[:, n].sum())
        emitted += c
        src = scores[:, n].reshape(-1)[torch.from_numpy(ei)]
        decayed += int((_bits(src[~nan]) != _bits(es[~nan])).sum())
    return cand, emitted, decayed


VQ = [(1, 1), (2, 5), (2, 300), (4, 300), (7, 300), (4, 1024)]


@pytest.mark.parametrize("V,Q", VQ)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tta_merge_matches_the_reference(dtype, mode, V, Q):
    """every label layout per case; N, the counts and the flip mask rotate with the layout and the case"""
    case = VQ.index((V, Q))
    for li, layout in enumerate(LAYOUTS):
        if (V, Q) == (4, 1024) and layout == "one" and dtype != torch.float32:
            continue    # 4096 candidates in one chain: once per mode, in f32 (the reference's slowest case)
        N = 3 if (li + case) % 2 == 0 else 1
        flip_kind = FLIPS[(li + case + MODES.index(mode)) % 3]
        full = li % 2 == 1
        if (V, Q) == (4, 1024):
            N, full = 1, True                              # exactly at the cap, every slot a candidate
        cand, emitted, decayed = _merge_and_compare(dtype, mode, V, N, Q, layout, flip_kind, full,
                                                    seed=100 * case + 10 * li + MODES.index(mode))
        if V * Q >= 10 and layout != "own" and cand >= 10:
            # near and exact duplicates across views share a label: something must go or decay
            assert emitted < cand or decayed > 0, (layout, cand, emitted, decayed)
        if layout == "own" and mode == "nms":
            assert emitted == cand                          # no two candidates share a label


@pytest.mark.parametrize("mode", MODES)
def test_tta_merge_every_flip_mask_and_both_batch_sizes(mode):
    for flip_kind in FLIPS:
        for N in (1, 3):
            for full in (True, False):
                _merge_and_compare(torch.float16, mode, 3, N, 40, "two", flip_kind, full, seed=7 + N)


@pytest.mark.parametrize("mode", MODES)
def test_tta_merge_max_per_img(mode):
    for keep in (1, 17, 100, 5000):      # 5000 > V * Q: K follows max_keep, the rows beyond the count are zero
        _merge_and_compare(torch.float32, mode, 2, 3, 50, "eighty", "alternating", True, seed=3, max_per_img=keep)


def test_unflip_tie_and_threshold_rules_on_the_gpu():
    """the four hand-made cases a wrong un-flip, `>=` for `>` or a reversed tie rule would change"""
    from codetr import hip_ops

    def run(boxes, scores, flips, width, nms):
        V = len(boxes)
        dets = [hip_ops.Detections(torch.tensor([[boxes[v]]], dtype=torch.float32, device=DEV),
                                   torch.tensor([[scores[v]]], dtype=torch.float32, device=DEV),
                                   torch.zeros((1, 1), dtype=torch.int64, device=DEV),
                                   torch.ones((1,), dtype=torch.int32, device=DEV), None) for v in range(V)]
        h = hip_ops.detections_to_host(hip_ops.tta_merge(dets, flips, [width], nms))
        c = int(h.count[0])
        return h.index[0, :c].tolist(), h.scores[0, :c].tolist(), h.boxes[0, :c].tolist()

    hard = dict(type="nms", iou_threshold=0.5)
    # two views of one box, one flipped: one detection, and the flipped view's box comes back un-flipped
    assert run([[10, 20, 40, 60], [60, 20, 90, 60]], [0.9, 0.8], [False, True], 100.0, hard)[0] == [0]
    idx, sc, bx = run([[10, 20, 40, 60], [60, 20, 90, 60]], [0.8, 0.9], [False, True], 100.0, hard)
    assert idx == [1] and bx == [[10.0, 20.0, 40.0, 60.0]]
    idx, sc, bx = run([[500, 0, 510, 10], [60, 20, 95, 60]], [0.8, 0.9], [False, True], 100.0, hard)
    assert idx == [1, 0] and bx[0] == [5.0, 20.0, 40.0, 60.0]                 # (W - x2, y1, W - x1, y2)
    # linear soft-NMS decays the second view: IoU 0.75
    idx, sc, _ = run([[10, 20, 40, 60], [60, 20, 100, 60]], [0.9, 0.8], [False, True], 100.0,
                     dict(type="soft_nms", iou_threshold=0.3, method="linear"))
    assert idx == [0, 1] and sc[1] == float(np.float32(0.8) * np.float32(0.25))
    # IoU exactly at the threshold: hard NMS keeps both
    assert run([[0, 0, 2, 2], [0, 0, 2, 1]], [0.5, 0.4], [False, False], 10.0, hard)[0] == [0, 1]
    assert run([[0, 0, 2, 2], [0, 0, 2, 1]], [0.5, 0.4], [False, False], 10.0, dict(type="nms", iou_threshold=0.49))[0] == [0]
    # equal scores: the lower c is picked first and suppresses the other; apart, the lower c is listed first
    assert run([[0, 0, 2, 2], [0, 0, 2, 1.5]], [0.5, 0.5], [False, False], 10.0, hard)[0] == [0]
    assert run([[0, 0, 2, 2], [5, 5, 6, 6]], [0.5, 0.5], [False, False], 10.0, hard)[0] == [0, 1]


ONE_VIEW = [(dt, Q, False) for dt in DTYPES for Q in (1, 65, 300)] + [(torch.float32, 1024, True)]


@pytest.mark.parametrize("method", ["linear", "naive"])
@pytest.mark.parametrize("dtype,Q,one_label", ONE_VIEW)
def test_one_view_merge_equals_the_soft_postprocess(dtype, Q, one_label, method):
    """GPU against GPU: the merge of ONE unflipped view with every row a candidate is the soft-NMS post-processing of
    that view with unit divisors and no score threshold -- both kernels are their own front end followed by the same
    sort, segment, chain and row-writing code.  count and all Q rows of index, labels, scores and boxes, bit for bit.
    Q = 1024 under one label is 16 positions per lane in both (a 32-bit mask in one, a 64-bit mask in the other)."""
    from codetr import hip_ops
    from test_softnms_gpu import _image

    N, t = 2, 0.8 if one_label else 0.5
    rng = np.random.default_rng(1200 + Q)
    layouts = ("one", "one") if one_label else ("one", "mixed")      # ties, zero scores, zero-area pairs; no NaN
    images = [_image(rng, Q, layout, one_label or i == 0, dtype) for i, layout in enumerate(layouts)]
    boxes = torch.stack([im[0] for im in images]).to(DEV)
    scores = torch.stack([im[1] for im in images]).to(DEV)
    labels = torch.from_numpy(np.stack([im[2] for im in images])).to(DEV)
    view = hip_ops.Detections(boxes, scores, labels, torch.full((N,), Q, dtype=torch.int32, device=DEV), None)
    merged = hip_ops.detections_to_host(hip_ops.tta_merge(
        [view], [False], [1000.0] * N, dict(type="soft_nms", iou_threshold=t, method=method, min_score=1e-3), None))
    soft = hip_ops.detections_to_host(hip_ops.postprocess_detections_soft(
        boxes, scores, labels, torch.ones((N, 4), dtype=dtype, device=DEV), None, t, method, 1e-3, None))
    print(f"{dtype} Q={Q} {method}: counts {merged.count.tolist()} / {soft.count.tolist()}")
    assert merged.scores.shape == soft.scores.shape == (N, Q)
    assert merged.count.tolist() == soft.count.tolist()
    if Q >= 65:
        assert all(0 < c < Q for c in soft.count.tolist())             # something was picked, something left
    assert torch.equal(merged.index, soft.index) and torch.equal(merged.labels, soft.labels)
    assert torch.equal(_bits(merged.scores), _bits(soft.scores)) and torch.equal(_bits(merged.boxes), _bits(soft.boxes))


def test_tta_merge_host_side_limits():
    from codetr import hip_ops

    def dets(rows, Q):
        return hip_ops.Detections(torch.zeros((rows, Q, 4), device=DEV), torch.zeros((rows, Q), device=DEV),
                                  torch.zeros((rows, Q), dtype=torch.int64, device=DEV),
                                  torch.zeros((rows,), dtype=torch.int32, device=DEV), None)

    with pytest.raises(ValueError, match="4096"):
        hip_ops.tta_merge([dets(1, 1025)] * 4 + [dets(1, 1025)], [False] * 5, [10.0])
    with pytest.raises(ValueError, match="16"):
        hip_ops.tta_merge([dets(17, 2)], [False] * 17, [10.0])
    with pytest.raises(ValueError):
        hip_ops.tta_merge([dets(2, 5)], [False], [10.0])                      # two views, one flag
    with pytest.raises(NotImplementedError):
        hip_ops.tta_merge([dets(1, 5)], [False], [10.0], dict(type="soft_nms", method="gaussian"))
    out = hip_ops.detections_to_host(hip_ops.tta_merge([dets(2, 5)], [False, True], [10.0]))
    assert int(out.count[0]) == 0 and out.scores.shape == (1, 10)             # counts of zero: nothing to merge


# ---- 3. end to end ------------------------------------------------------------------------------------------------
TTA = dict(scales=[(320, 200), (400, 256)], flip=True)


def _stub(seen, Q=64):
    """detections from the middle row of each view's own input (the `_row_model` pattern, for small views)"""
    def model(x, m):
        seen.append(tuple(x.shape))
        H, W = x.shape[2:]
        r = x[:, :, H // 2, :].float()[:, :, torch.arange(3 * Q, device=x.device) % W]
        scores = torch.sigmoid(r[:, 0, :Q] * 2)
        c = torch.stack((r[:, 1, :Q] * 40 + 150, r[:, 2, :Q] * 30 + 100), -1)
        wh = torch.stack((r[:, 0, Q:2 * Q].abs() * 40 + 20, r[:, 1, Q:2 * Q].abs() * 40 + 20), -1)
        labels = (r[:, 2, 2 * Q:].abs() * 10).long() % 3
        return torch.cat((c - wh / 2, c + wh / 2), -1).to(x.dtype), scores.to(x.dtype), labels
    return model


def _inferencer(model, tta, **kw):
    from codetr.inferencer import Inferencer

    return Inferencer(model, SWIN, dataset_meta=None, tta=tta, **kw)


def _composed(inf, model, images, dtype, batch_size):
    """the TTA call restated without the Inferencer's own TTA methods: the row table from rescale_size and the divisor
    rule written out here, hip_ops.preprocess_views, the model, the existing post-processing launch and tta_ref per image
    -> (result dicts, the batch shapes the model must have seen)"""
    from codetr import hip_ops
    from codetr.inferencer import rescale_size

    t, out, shapes = inf.tta, [], []
    flips = (False, True) if t["flip"] else (False,)
    mode = "nms" if t["nms"]["type"] == "nms" else t["nms"]["method"]
    ts = _to_storage(dtype)
    d = inf.pad_size_divisor
    for start in range(0, len(images), batch_size):
        chunk = images[start:start + batch_size]
        N = len(chunk)
        src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in chunk])).to(DEV)
        offsets = np.cumsum([0] + [im.size for im in chunk]).tolist()
        per_view = []
        for scale in t["scales"]:
            rows, div = [], []
            for f in flips:                                   # flip-major: row f * N + n
                for o, im in zip(offsets, chunk):
                    H, W = im.shape[:2]
                    nh, nw = rescale_size(H, W, scale)
                    rows.append((o, H, W, nh, nw, nh, nw, int(f)))
                    div.append([nw / W, nh / H, nw / W, nh / H])
            Hb = max(-(-r[3] // d) * d for r in rows)
            Wb = max(-(-r[4] // d) * d for r in rows)
            shapes.append((len(rows), 3, Hb, Wb))
            x, m = hip_ops.preprocess_views(src, rows, (Hb, Wb), inf.mean, inf.std, inf.pad_val, inf.pad_value, dtype)
            with torch.no_grad():
                boxes, scores, labels = model(x, m)
            div = torch.tensor(div, dtype=dtype).to(DEV)
            thr = inf.score_threshold if inf.score_threshold > 0 else None
            if inf.soft:
                dets = hip_ops.postprocess_detections_soft(boxes, scores, labels, div, thr, inf.iou_threshold,
                                                           inf.soft_method, inf.min_score, inf.max_per_img)
            else:
                dets = hip_ops.postprocess_detections(boxes, scores, labels, div, thr, inf.iou_threshold)
            h = hip_ops.detections_to_host(dets)
            Q = h.scores.shape[1]
            per_view.append((h.boxes.view(len(flips), N, Q, 4), h.scores.view(len(flips), N, Q),
                             h.labels.view(len(flips), N, Q), h.count.view(len(flips), N)))
        b, s, l, c = (torch.cat([v[i] for v in per_view]) for i in range(4))   # v = s * flips + f
        view_flips = [f for _ in t["scales"] for f in flips]
        for n, im in enumerate(chunk):
            eb, es, el, _ = R.merge_outputs(b[:, n].float().numpy(), s[:, n].float().numpy(), l[:, n].numpy(),
                                            c[:, n].numpy(), view_flips, float(im.shape[1]), ts, mode,
                                            t["nms"]["iou_threshold"], t["nms"]["min_score"], t["max_per_img"] or 0)
            out.append({"labels": el.tolist(), "scores": es.float().tolist(), "bboxes": eb.float().tolist()})
    return out, shapes


def test_view_rows_known_answers():
    """the row table, scale factors and divisor padding of one scale, by hand: 480x640 into (320, 200) is 200x267
    (factor min(320/640, 200/480) = 0.41667: 200.0 x 266.67 -> 267), 100x1000 is 32x320; padded to 32: 224x288 and
    32x320, so the batch is 224x320"""
    inf = _inferencer(None, dict(scales=[(320, 200)], flip=True))
    inf.pad_size_divisor = 32
    rows, metas, hw = inf.view_rows([0, 921600], [(480, 640), (100, 1000)], (320, 200), (False, True))
    assert rows == [(0, 480, 640, 200, 267, 200, 267, 0), (921600, 100, 1000, 32, 320, 32, 320, 0),
                    (0, 480, 640, 200, 267, 200, 267, 1), (921600, 100, 1000, 32, 320, 32, 320, 1)]
    assert hw == (224, 320) and [m["pad_shape"] for m in metas] == [(224, 288), (32, 320)] * 2
    assert [m["flip"] for m in metas] == [False, False, True, True]
    assert metas[0]["scale_factor"] == (267 / 640, 200 / 480) and metas[3]["scale_factor"] == (320 / 1000, 32 / 100)
    assert all(m["batch_input_shape"] == (224, 320) for m in metas)
    assert inf.divisors(metas[:1], torch.float32).tolist() == [[np.float32(267 / 640), np.float32(200 / 480)] * 2]


@pytest.mark.parametrize("dtype,nms,nms_type", [
    (torch.float32, dict(type="nms", iou_threshold=0.5), None),
    (torch.float16, dict(type="soft_nms", iou_threshold=0.4, method="linear", min_score=0.05), "soft_nms"),
    (torch.bfloat16, dict(type="soft_nms", iou_threshold=0.4, method="naive"), None)])
def test_tta_inferencer_equals_the_composition_with_a_stub_model(dtype, nms, nms_type):
    from codetr import _cabi

    seen = []
    model = _stub(seen)
    inf = _inferencer(model, dict(TTA, nms=nms, max_per_img=50), score_threshold=0.3, nms_type=nms_type)
    inf.pad_size_divisor, inf.pad_value = 32, 0.5          # (no shipped config sets one: exercise the divisor padding)
    post = "postprocess_softnms" if inf.soft else "postprocess_detections"
    images = _images([(480, 640), (1333, 2000), (37, 53), (768, 1152), (600, 900)], 23)
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=dtype, batch_size=2)["predictions"]
    after = dict(_cabi.CALLS)
    # three chunks: per chunk one preprocess_views and one post-processing launch per scale, one merge
    assert after["preprocess_views"] - before["preprocess_views"] == 3 * 2
    assert after[post] - before[post] == 3 * 2
    assert after["tta_merge"] - before["tta_merge"] == 3
    assert after["preprocess_batch"] == before["preprocess_batch"] and after["preprocess"] == before["preprocess"]
    assert [s[0] for s in seen] == [4, 4, 4, 4, 2, 2] and inf.num_predicted_imgs == 5
    assert all(s[2] % 32 == 0 and s[3] % 32 == 0 and s[2] <= 256 and s[3] <= 416 for s in seen)
    by_inferencer = list(seen)
    expect, shapes = _composed(inf, model, images, dtype, 2)
    assert by_inferencer == shapes
    _same(got, expect)
    assert 10 < sum(len(p["labels"]) for p in got) and all(len(p["labels"]) <= 50 for p in got)
    # the same images without TTA: neither new entry point is called
    plain = _inferencer(model, None, score_threshold=0.3)
    before = dict(_cabi.CALLS)
    plain(images, device=DEV, dtype=dtype, batch_size=2)
    assert _cabi.CALLS["preprocess_views"] == before["preprocess_views"]
    assert _cabi.CALLS["tta_merge"] == before["tta_merge"]
    assert _cabi.CALLS["preprocess_batch"] == before["preprocess_batch"] + 3


def test_tta_inferencer_rejects_more_than_4096_candidates():
    inf = _inferencer(_stub([], Q=600), dict(scales=[(320, 200)] * 4, flip=True))
    with pytest.raises(ValueError, match="4096"):
        inf(_images([(48, 64)], 24), device=DEV, batch_size=1)


def test_tta_inferencer_with_the_tiny_model():
    import codetr
    from codetr import _cabi
    from helpers_model import seeded_params
    from test_model_gpu import _tiny_codetr_cfg

    dtype = torch.float16
    torch.manual_seed(0)
    model = codetr.CoDETR(**_tiny_codetr_cfg("swin"))
    spec = [(k, tuple(v.shape)) for k, v in model.named_parameters()]
    full = dict(model.state_dict())
    full.update(seeded_params(spec, 77, scale=1.5))
    model.load_state_dict(full)
    model = model.to(DEV, dtype).eval()
    inf = _inferencer(model, dict(TTA, nms=dict(type="nms", iou_threshold=0.6), max_per_img=100))
    images = _images([(480, 640), (300, 1000), (777, 555)], 25)
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=dtype, batch_size=2)["predictions"]
    assert _cabi.CALLS["preprocess_views"] - before["preprocess_views"] == 4
    assert _cabi.CALLS["tta_merge"] - before["tta_merge"] == 2
    _same(got, _composed(inf, model, images, dtype, 2)[0])
    assert len(got) == 3 and sum(len(p["labels"]) for p in got) > 0
