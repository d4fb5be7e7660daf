"""GPU: sliced inference in the Inferencer -- codetr_preprocess_tiles_u8_* against the oracle's preprocessing and
preprocess_batch of the contiguous crop, codetr_slice_merge_* bit for bit against the numpy restatement of its header
text (tests/slice_ref.py), and `Inferencer(slicing=...)` against the composition of its steps."""
import numpy as np
import pytest
import torch

import inferencer_ref as O
import slice_ref as R
from test_inferencer_batch_gpu import DEV, SWIN, _bits, _images, _same
from test_tta_gpu import _stub, _to_storage

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MEAN, STD, PAD_VAL, FILL = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375), (114, 7, 250), 0.5


def _f32(t):
    """a CPU tensor's values widened to fp32 exactly, NaN sign and payload included, as the kernels' own conversion does
    (Tensor.float() on the host is not bit-faithful for NaN: its vector and scalar paths give different payloads, and
    the payload is part of the sort key)"""
    if t.dtype == torch.float32:
        return t.contiguous().numpy()
    bits = t.contiguous().view(torch.int16).numpy()
    if t.dtype == torch.float16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.view(np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- 1. preprocessing of tiles ------------------------------------------------------------------------------------
def _crops(H, W):
    """(y0, x0, h, w): the top-left corner, the interior, flush with the right and bottom edges, one pixel wide, all"""
    return [(0, 0, H // 2, W // 3), (H // 4, W // 5, H // 2 + 1, W // 2), (H - H // 3, W - W // 2, H // 3, W // 2),
            (3, W - 1, H - 5, 1), (0, 0, H, W)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_preprocess_tiles_equals_the_contiguous_crop(dtype):
    """20 rows over two images in one launch: every crop once upscaled and once downscaled; each row against the
    oracle's preprocessing of the contiguous crop (no Pad region) and, with a Pad region and a margin, against
    preprocess_batch of that crop uploaded on its own"""
    from codetr import _cabi, hip_ops
    from codetr.inferencer import rescale_size

    images = _images([(53, 37), (96, 64)], 31)
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    offsets = [0, images[0].size]
    rows, plain, crops, scales = [], [], [], []
    for factor in (1.7, 0.6):            # a (long, short) bound pair per crop: every crop is resized by about `factor`
        for im, off in zip(images, offsets):
            H, W = im.shape[:2]
            for y0, x0, h, w in _crops(H, W):
                scale = (int(np.ceil(factor * max(h, w))), int(np.ceil(factor * min(h, w))))
                nh, nw = rescale_size(h, w, scale)
                assert nh >= 1 and nw >= 1 and ((nh > h or nw > w) if factor > 1 else (nh < h or nw < w))
                rows.append((off, H, W, y0, x0, h, w, nh, nw, nh + 3, nw + 5))
                plain.append((off, H, W, y0, x0, h, w, nh, nw, nh, nw))
                crops.append(np.ascontiguousarray(im[y0:y0 + h, x0:x0 + w]))
                scales.append(scale)
    assert len(rows) == 20 and any(r[6] == 1 for r in rows)
    Hb, Wb = max(r[9] for r in rows) + 2, max(r[10] for r in rows) + 1
    before = dict(_cabi.CALLS)
    x, m = hip_ops.preprocess_tiles(src, rows, (Hb, Wb), MEAN, STD, PAD_VAL, FILL, dtype)
    xp, mp = hip_ops.preprocess_tiles(src, plain, (Hb, Wb), MEAN, STD, PAD_VAL, FILL, dtype)
    assert _cabi.CALLS["preprocess_tiles"] == before["preprocess_tiles"] + 2
    assert _cabi.CALLS["preprocess_batch"] == before["preprocess_batch"]
    assert x.shape == (20, 3, Hb, Wb) and m.shape == (20, Hb, Wb) and x.dtype == m.dtype == dtype
    for i, (crop, scale) in enumerate(zip(crops, scales)):
        h, w = crop.shape[:2]
        nh, nw = rows[i][7:9]
        own = torch.from_numpy(crop.reshape(-1)).to(DEV)
        xb, mb = hip_ops.preprocess_batch(own, [(0, h, w, nh, nw, nh + 3, nw + 5)], (Hb, Wb), MEAN, STD, PAD_VAL, FILL, dtype)
        assert torch.equal(_bits(x[i]), _bits(xb[0])) and torch.equal(_bits(m[i]), _bits(mb[0])), (i, rows[i])
        ox, om, meta = O.preprocess(crop, scale, (0, 0), MEAN, STD, PAD_VAL)
        assert meta["img_shape"] == (nh, nw)
        assert torch.equal(_bits(xp[i, :, :nh, :nw]), _bits(torch.from_numpy(ox).to(dtype))), (i, plain[i])
        assert torch.equal(_bits(mp[i, :nh, :nw]), _bits(torch.from_numpy(om).to(dtype)))
        assert bool((mp[i, nh:] == 1).all()) and bool((mp[i, :, nw:] == 1).all())
        assert bool((xp[i, :, nh:] == FILL).all()) and bool((xp[i, :, :, nw:] == FILL).all())


def test_preprocess_tiles_splits_more_than_32_rows():
    from codetr import _cabi, hip_ops

    img = _images([(20, 30)], 32)[0]
    src = torch.from_numpy(img.reshape(-1)).to(DEV)
    rows = [(0, 20, 30, i % 5, i % 7, 15, 23, 40, 60, 40, 60) for i in range(33)]
    before = _cabi.CALLS["preprocess_tiles"]
    x, _ = hip_ops.preprocess_tiles(src, rows, (64, 64), (0, 0, 0), (1, 1, 1), dtype=torch.float16)
    assert _cabi.CALLS["preprocess_tiles"] == before + 2
    own = torch.from_numpy(np.ascontiguousarray(img[2:17, 4:27]).reshape(-1)).to(DEV)      # row 32: y0 = 2, x0 = 4
    xb, _ = hip_ops.preprocess_batch(own, [(0, 15, 23, 40, 60, 40, 60)], (64, 64), (0, 0, 0), (1, 1, 1), dtype=torch.float16)
    assert torch.equal(_bits(x[32]), _bits(xb[0]))
    assert not torch.equal(_bits(x[0]), _bits(x[1]))
    with pytest.raises(ValueError):
        hip_ops.preprocess_tiles(src, [r[:8] for r in rows], (64, 64), (0, 0, 0), (1, 1, 1))


# ---- 2. the merge -------------------------------------------------------------------------------------------------
SIZES = [[1000.0, 700.0], [640.0, 480.0], [333.0, 517.0]]            # (W, H)


def _inputs(dtype, V, N, Q, one_label, seed):
    """the stacked per-row detections of N images of V views (CPU tensors), R = N V + 2 rows in a shuffled order: every
    view sees the image's Q objects slightly moved, in its own crop's coordinates (near duplicates across views); boxes
    straddling and wholly outside the image, a NaN coordinate, zero-area boxes, tied, zero and NaN scores, ragged and
    zero counts, absent views"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.tensor(SIZES[:N])
    Rn = N * V + 2
    rows = torch.randperm(Rn, generator=g)[:N * V].view(N, V).to(torch.int32)
    origins = torch.zeros(Rn, 2)
    boxes, scores = torch.zeros(Rn, Q, 4), torch.rand(Rn, Q, generator=g)
    labels = torch.zeros(Rn, Q, dtype=torch.int64)
    count = torch.full((Rn,), Q, dtype=torch.int32)
    for n in range(N):
        c = (torch.rand(Q, 2, generator=g) * 1.3 - 0.15) * sizes[n]              # some centres outside the image
        wh = torch.rand(Q, 2, generator=g) * 150 + 2
        base = torch.cat((c - wh / 2, c + wh / 2), -1)
        if Q > 12:
            base[7:10, 2] = base[7:10, 0]                                         # zero-area boxes
            base[10:12] = base[7:9]                                               # ... and their duplicates
        lab = torch.full((Q,), 5) if one_label else torch.randint(0, 3, (Q,), generator=g) * 40 - 3
        tied = torch.rand(Q, generator=g)
        for v in range(V):
            r = int(rows[n, v])
            if v > 0:
                origins[r] = torch.floor(torch.rand(2, generator=g) * sizes[n] * 0.8)
            boxes[r] = base - origins[r].repeat(2) + (torch.rand(Q, 4, generator=g) - 0.5) * 6
            if v == 1:
                boxes[r, ::5] = boxes[int(rows[n, 0]), ::5] - origins[r].repeat(2)   # the same boxes in the image
            scores[r, ::3] = tied[::3]                                            # ties across views: the lowest c decides
            scores[r, 1::7] = scores[r, 0]                                        # ... and inside a view
            labels[r] = lab
            if not one_label and v == 0:
                labels[r, ::11] = 37                                              # views may disagree
            if Q > 6:
                boxes[r, 5] += 5000.0                                             # wholly outside: clipped to nothing
                scores[r, 2] = -0.0
                scores[r, 3] = 0.0
            if (n + v) % 3 == 1:
                count[r] = int(torch.randint(0, Q + 1, (1,), generator=g))        # ragged
    if Q > 4:
        boxes[int(rows[0, V - 1]), 4, 1] = float("nan")
        scores[int(rows[0, 0]), 4] = float("nan")
    if V > 2:
        count[int(rows[0, V - 1])] = 0                                            # a view with nothing
        rows[0, V // 2] = -1                                                      # absent views
    if N == 3:
        rows[1, 0] = Rn
        count[rows[2].long()] = 0                                                 # an image with nothing
    return boxes.to(dtype), scores.to(dtype), labels, count, rows, origins, sizes


def _merge_and_compare(dtype, V, N, Q, one_label, seed, merge, max_per_img=None, zero_counts=False):
    """-> (candidates, emitted, grown boxes) summed over the images"""
    from codetr import _cabi, hip_ops

    boxes, scores, labels, count, rows, origins, sizes = _inputs(dtype, V, N, Q, one_label, seed)
    if zero_counts:
        count[:] = 0
    dets = hip_ops.Detections(boxes.to(DEV), scores.to(DEV), labels.to(DEV), count.to(DEV), None)
    before = _cabi.CALLS["slice_merge"]
    out = hip_ops.slice_merge(dets, rows.to(DEV), origins.to(DEV), sizes.to(DEV), merge, max_per_img)
    assert _cabi.CALLS["slice_merge"] == before + 1
    host = hip_ops.detections_to_host(out)
    K = max_per_img if max_per_img else V * Q
    assert host.scores.shape == (N, K) and host.boxes.shape == (N, K, 4) and host.index.shape == (N, K)
    ts = _to_storage(dtype)
    cand = emitted = grown = 0
    fb, fs = _f32(boxes), _f32(scores)
    for n in range(N):
        eb, es, el, ei = R.merge_outputs(fb, fs, labels.numpy(), count.numpy(), rows[n].tolist(), origins.numpy(),
                                         sizes[n].tolist(), ts, metric=merge["metric"], mode=merge["type"],
                                         threshold=merge["threshold"], class_agnostic=merge["class_agnostic"],
                                         max_keep=max_per_img or 0)
        c = int(host.count[n])
        here = sum(int(count[r]) for r in rows[n].tolist() if 0 <= r < len(count))
        print(f"{dtype} {merge} V={V} Q={Q} n={n}: candidates {here} -> {c}")
        assert c == len(ei)
        assert host.index[n, :c].tolist() == ei.tolist()
        assert host.labels[n, :c].tolist() == el.tolist()
        assert torch.equal(_bits(host.boxes[n, :c]), _bits(eb))
        gs, nan = host.scores[n, :c], torch.isnan(es)
        assert torch.equal(torch.isnan(gs), nan) and torch.equal(_bits(gs[~nan]), _bits(es[~nan]))
        assert bool((host.labels[n, c:] == 0).all()) and bool((host.index[n, c:] == 0).all())
        assert bool((_bits(host.scores[n, c:]) == 0).all()) and bool((_bits(host.boxes[n, c:]) == 0).all())
        cand += here
        emitted += c
        if c:   # a pick's own box, shifted and clipped, against what was emitted for it
            picked = [(int(rows[n, int(i) // Q]), int(i) % Q) for i in ei]
            own = np.concatenate([R.shift_clip(fb[r, j], origins[r].numpy(), sizes[n].tolist()) for r, j in picked])
            grown += int((_bits(ts(own)) != _bits(eb)).any(-1).sum())
    return cand, emitted, grown


VQ = [(1, 1), (2, 64), (5, 300), (4, 256), (16, 256)]     # (4, 256): 1024 slots, the last under the 32-bit alive mask;
                                                           # (16, 256): 4096, the cap


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("metric", ["ios", "iou"])
@pytest.mark.parametrize("mode", ["nmm", "nms"])
@pytest.mark.parametrize("V,Q", VQ)
@pytest.mark.parametrize("dtype", DTYPES)
def test_slice_merge_matches_the_reference(dtype, V, Q, mode, metric, agnostic):
    """N = 1 and 3 and the label layout rotate with the case; one label throughout at the two slot-count steps, so that
    a chain holds exactly 16 and 64 positions per lane there"""
    case = VQ.index((V, Q)) + (mode == "nms") + 2 * (metric == "iou") + DTYPES.index(dtype)
    N = 3 if case % 2 == 0 else 1
    one_label = (case // 2) % 2 == 0 or (V, Q) in ((4, 256), (16, 256))
    merge = dict(type=mode, metric=metric, threshold=0.5 if metric == "ios" else 0.3, class_agnostic=agnostic)
    cand, emitted, grown = _merge_and_compare(dtype, V, N, Q, one_label, seed=10 * case + agnostic, merge=merge)
    if V * Q >= 100:
        assert 0 < emitted < cand                               # near duplicates across views: something was retired
        assert (grown > 0) == (mode == "nmm")                   # ... and, merging, absorbed


@pytest.mark.parametrize("mode", ["nmm", "nms"])
def test_slice_merge_max_per_img_and_nothing_to_merge(mode):
    merge = dict(type=mode, metric="ios", threshold=0.5, class_agnostic=False)
    for keep in (1, 17, 5000):           # 5000 > V * Q: K follows max_keep, the rows beyond the count are zero
        _merge_and_compare(torch.float16, 3, 3, 50, False, 3, merge, max_per_img=keep)
    for N in (1, 3):
        assert _merge_and_compare(torch.float32, 3, N, 50, False, 4, merge, zero_counts=True)[:2] == (0, 0)


def test_slice_merge_rules_on_the_gpu():
    """the hand-made cases of tests/test_slice_cpu.py on the device: IoS against IoU, the union against the pick's own
    box, `>` not `>=`, the tie rule, the origin shift, the clip and the box of no area"""
    from codetr import hip_ops

    def run(boxes, scores, origin=(0.0, 0.0), labels=(1, 1, 1), **merge):
        n = len(boxes)
        dets = hip_ops.Detections(torch.tensor([boxes], dtype=torch.float32, device=DEV),
                                  torch.tensor([scores], dtype=torch.float32, device=DEV),
                                  torch.tensor([labels[:n]], dtype=torch.int64, device=DEV),
                                  torch.tensor([n], dtype=torch.int32, device=DEV), None)
        h = hip_ops.detections_to_host(hip_ops.slice_merge(dets, [[0]], [list(origin)], [[100.0, 100.0]], merge))
        c = int(h.count[0])
        return h.index[0, :c].tolist(), h.boxes[0, :c].tolist()

    inside = [[0, 0, 40, 40], [10, 10, 20, 20], [60, 60, 80, 80]]
    assert run(inside, [0.9, 0.8, 0.7], type="nms", metric="iou")[0] == [0, 1, 2]
    assert run(inside, [0.9, 0.8, 0.7], type="nms", metric="ios")[0] == [0, 2]
    assert run(inside, [0.9, 0.8, 0.7], labels=(1, 2, 1), type="nms")[0] == [0, 1, 2]
    assert run(inside, [0.9, 0.8, 0.7], labels=(1, 2, 1), type="nms", class_agnostic=True)[0] == [0, 2]
    chain = [[10, 10, 30, 30], [20, 5, 35, 25], [32, 0, 50, 10]]
    assert run(chain, [0.9, 0.8, 0.7], threshold=0.4) == ([0, 2], [[10, 5, 35, 30], [32, 0, 50, 10]])
    assert run(chain, [0.9, 0.8, 0.7], threshold=0.5) == ([0, 1, 2], [[float(v) for v in b] for b in chain])
    assert run(chain, [0.8, 0.9, 0.7], threshold=0.4) == ([1, 2], [[10, 5, 35, 30], [32, 0, 50, 10]])
    assert run(chain, [0.8, 0.8, 0.8], threshold=0.4)[0] == [0, 2]
    edge = [[-5, -5, 5, 3], [20, 20, 30, 30], [20, 20, 30, 30]]
    for merge in (dict(type="nms", metric="iou"), dict(type="nmm", metric="ios")):
        assert run(edge, [0.9, 0.8, 0.7], origin=(90.0, 95.0), threshold=0.0, **merge) == (
            [0, 1, 2], [[85, 90, 95, 98], [100, 100, 100, 100], [100, 100, 100, 100]])
    assert run([[float("nan"), -3, 7, 200]], [0.5], origin=(1.0, 2.0))[1] == [[0, 0, 8, 100]]


def test_slice_merge_host_side_limits():
    from codetr import hip_ops

    def dets(rows, Q):
        return hip_ops.Detections(torch.zeros((rows, Q, 4), device=DEV), torch.zeros((rows, Q), device=DEV),
                                  torch.zeros((rows, Q), dtype=torch.int64, device=DEV),
                                  torch.zeros((rows,), dtype=torch.int32, device=DEV), None)

    with pytest.raises(ValueError, match="4096"):
        hip_ops.slice_merge(dets(5, 1025), [[0, 1, 2, 3, 4]], [[0, 0]] * 5, [[10, 10]])
    with pytest.raises(ValueError, match="64"):
        hip_ops.slice_merge(dets(65, 2), [list(range(65))], [[0, 0]] * 65, [[10, 10]])
    with pytest.raises(ValueError):
        hip_ops.slice_merge(dets(2, 5), [[0, 1]], [[0, 0]], [[10, 10]])             # two rows, one origin
    with pytest.raises(ValueError, match="metric"):
        hip_ops.slice_merge(dets(1, 5), [[0]], [[0, 0]], [[10, 10]], dict(metric="giou"))
    out = hip_ops.detections_to_host(hip_ops.slice_merge([dets(1, 5), dets(1, 5)], [[0, 1]], [[0, 0]] * 2, [[10, 10]]))
    assert int(out.count[0]) == 0 and out.scores.shape == (1, 10)                  # counts of zero: nothing to merge


# ---- 3. end to end ------------------------------------------------------------------------------------------------
def _inferencer(model, slicing, divisor=(32, 0.5), **kw):
    from codetr.inferencer import Inferencer

    inf = Inferencer(model, SWIN, dataset_meta=None, slicing=slicing, **kw)
    inf.scale = (400, 256)          # (small views: the shipped scale would make every 256-tile a 768 x 768 input)
    inf.pad_size_divisor, inf.pad_value = divisor   # (no shipped config sets one: exercise the divisor padding)
    return inf


def _composed(inf, model, images, dtype, batch_size):
    """the sliced call restated without the Inferencer's own slicing methods: the grid from slice_ref, the row table,
    scale factors and divisor padding written out here, hip_ops.preprocess_tiles, the model over the same tile_batch
    groups, the existing post-processing launch and slice_ref per image -> (result dicts, the shapes the model saw)"""
    from codetr import hip_ops

    s, out, shapes = inf.slicing, [], []
    ts = _to_storage(dtype)
    d = inf.pad_size_divisor
    for start in range(0, len(images), batch_size):
        chunk = images[start:start + batch_size]
        src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in chunk])).to(DEV)
        offsets = np.cumsum([0] + [im.size for im in chunk]).tolist()
        rows, div, origins, table = [], [], [], []
        for o, im in zip(offsets, chunk):
            H, W = im.shape[:2]
            views = R.grid(H, W, s["tile"], s["overlap"]) + ([(0, 0, H, W)] if s["full_image"] else [])
            table.append(list(range(len(rows), len(rows) + len(views))))
            for y0, x0, h, w in views:
                nh, nw, _ = O.rescale_size(h, w, inf.scale)
                rows.append((o, H, W, y0, x0, h, w, nh, nw, nh, nw))
                div.append([nw / w, nh / h, nw / w, nh / h])
                origins.append([float(x0), float(y0)])
        Hb, Wb = max(-(-r[7] // d) * d for r in rows), max(-(-r[8] // d) * d for r in rows)
        x, m = hip_ops.preprocess_tiles(src, rows, (Hb, Wb), inf.mean, inf.std, inf.pad_val, inf.pad_value, dtype)
        div = torch.tensor(div, dtype=dtype).to(DEV)
        thr = inf.score_threshold if inf.score_threshold > 0 else None
        parts = []
        for i in range(0, len(rows), s["tile_batch"]):
            j = min(len(rows), i + s["tile_batch"])
            shapes.append((j - i, 3, Hb, Wb))
            with torch.no_grad():
                boxes, scores, labels = model(x[i:j], m[i:j])
            if inf.soft:
                dets = hip_ops.postprocess_detections_soft(boxes, scores, labels, div[i:j], thr, inf.iou_threshold,
                                                           inf.soft_method, inf.min_score, inf.max_per_img)
            else:
                dets = hip_ops.postprocess_detections(boxes, scores, labels, div[i:j], thr,
                                                      inf.iou_threshold if inf.with_nms else None)
            parts.append(hip_ops.detections_to_host(dets))
        b, sc, lab, cnt = (torch.cat([getattr(p, k) for p in parts]) for k in ("boxes", "scores", "labels", "count"))
        mg = s["merge"]
        for n, im in enumerate(chunk):
            eb, es, el, _ = R.merge_outputs(_f32(b), _f32(sc), lab.numpy(), cnt.numpy(), table[n],
                                            np.asarray(origins, np.float32), (im.shape[1], im.shape[0]), ts,
                                            metric=mg["metric"], mode=mg["type"], threshold=mg["threshold"],
                                            class_agnostic=mg["class_agnostic"], max_keep=s["max_per_img"] or 0)
            out.append({"labels": el.tolist(), "scores": es.float().tolist(), "bboxes": eb.float().tolist()})
    return out, shapes


@pytest.mark.parametrize("dtype,nms_type,full_image,tile_batch,merge", [
    (torch.float32, None, True, 4, dict(type="nmm", metric="ios", threshold=0.5)),
    (torch.float16, "soft_nms", False, 32, dict(type="nms", metric="iou", threshold=0.4, class_agnostic=True)),
    (torch.bfloat16, None, True, 32, dict(type="nmm", metric="iou", threshold=0.3)),
    (torch.float16, "soft_nms", False, 5, dict(type="nmm", metric="ios", threshold=0.5))])
def test_sliced_inferencer_equals_the_composition_with_a_stub_model(dtype, nms_type, full_image, tile_batch, merge):
    from codetr import _cabi

    seen = []
    model = _stub(seen)
    inf = _inferencer(model, dict(tile=(256, 256), overlap=0.25, full_image=full_image, merge=merge, max_per_img=40,
                                  tile_batch=tile_batch), score_threshold=0.3, nms_type=nms_type)
    assert inf.soft == (nms_type == "soft_nms")
    post = "postprocess_softnms" if inf.soft else "postprocess_detections"
    images = _images([(480, 640), (300, 333)], 33)
    # 3 x 3 tiles (x: 0, 192, 384; y: 0, 192, 224) and 2 x 2 (x: 0, 77; y: 0, 44), + the images
    R_rows = 9 + 4 + (2 if full_image else 0)
    forwards = -(-R_rows // tile_batch)
    before = dict(_cabi.CALLS)
    got = inf(images, device=DEV, dtype=dtype, batch_size=2)["predictions"]
    after = dict(_cabi.CALLS)
    assert after["slice_merge"] - before["slice_merge"] == 1
    assert after["preprocess_tiles"] - before["preprocess_tiles"] == -(-R_rows // 32) == 1
    assert after[post] - before[post] == forwards == len(seen)
    for k in ("preprocess_batch", "preprocess", "preprocess_views", "tta_merge"):
        assert after[k] == before[k], k
    assert sum(s[0] for s in seen) == R_rows and inf.num_predicted_imgs == 2
    by_inferencer = list(seen)
    expect, shapes = _composed(inf, model, images, dtype, 2)
    assert by_inferencer == shapes
    _same(got, expect)
    assert 10 < sum(len(p["labels"]) for p in got) and all(len(p["labels"]) <= 40 for p in got)
    # one image per chunk: its own rows only, stacked to its own batch shape
    one = inf(images, device=DEV, dtype=dtype, batch_size=1)["predictions"]
    _same(one, _composed(inf, model, images, dtype, 1)[0])


def test_slicing_none_leaves_the_plain_call_alone():
    from codetr import _cabi

    images = _images([(480, 640), (300, 333)], 33)
    plain = _inferencer(_stub([]), None, score_threshold=0.3)
    before = dict(_cabi.CALLS)
    plain(images, device=DEV, dtype=torch.float16, batch_size=2)
    after = dict(_cabi.CALLS)
    assert after["preprocess_tiles"] == before["preprocess_tiles"] and after["slice_merge"] == before["slice_merge"]
    assert after["preprocess_batch"] == before["preprocess_batch"] + 1
    assert after["postprocess_detections"] == before["postprocess_detections"] + 1
    assert {k for k in after if after[k] != before[k]} == {"preprocess_batch", "postprocess_detections"}


def test_sliced_inferencer_rejects_more_than_4096_candidates():
    inf = _inferencer(_stub([], Q=600), dict(tile=(256, 256), overlap=0.25))      # 9 tiles + the image, 600 each
    with pytest.raises(ValueError, match="4096"):
        inf(_images([(480, 640)], 34), device=DEV, batch_size=1)


def test_sliced_inferencer_with_the_tiny_model():
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
    # (the config's own padding: a margin of 0.5 in the whole-image row turns this random-weight model's scores to NaN)
    inf = _inferencer(model, dict(tile=(256, 256), tile_batch=8, max_per_img=100), divisor=(1, 0.0), visualizer=dict())
    images = _images([(480, 640), (300, 700)], 35)
    before = dict(_cabi.CALLS)
    res = inf(images, device=DEV, dtype=dtype, batch_size=2, return_vis=True)
    got = res["predictions"]
    assert _cabi.CALLS["slice_merge"] - before["slice_merge"] == 1
    assert _cabi.CALLS["preprocess_tiles"] - before["preprocess_tiles"] == 1
    assert _cabi.CALLS["draw_detections"] - before["draw_detections"] == 1
    assert [v.shape for v in res["visualization"]] == [im.shape for im in images]
    assert all(v.dtype == np.uint8 for v in res["visualization"])
    again = inf(images, device=DEV, dtype=dtype, batch_size=2)["predictions"]
    _same(got, again)
    _same(got, _composed(inf, model, images, dtype, 2)[0])
    assert len(got) == 2 and sum(len(p["labels"]) for p in got) > 0
    assert all(np.isfinite(p["scores"]).all() and np.isfinite(p["bboxes"]).all() for p in got)
