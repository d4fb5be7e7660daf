"""GPU: codetr_crop_detections_* (csrc/crops.hip) byte for byte against tests/crops_ref.py (no tolerance; the tensor form
bit for bit), and `Inferencer(crops=...)` with a stub model against the restatement applied to its own predictions."""
import numpy as np
import pytest
import torch

import crops_ref as R
import redact_cases as cases
from test_inferencer_batch_gpu import DEV, SWIN, _images, _same

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
PATTERN, GUARD = 0xA5, 4096   # the pre-fill of the outputs; bytes behind them that must keep it


def _run(dtype, buf, rows, boxes, scores, labels, count, st, select=None, tensor_dtype=None):
    """one codetr_crop_detections_* call into pre-filled outputs against the restatement: the slots below each count, and
    every other byte -- the source buffer, the slots beyond the counts, the guard regions -- unchanged -> the counts"""
    from codetr import _crops

    st = dict(R.DEFAULTS, **st)
    (w, h), M, N, pad = st["size"], st["max_per_img"], len(rows), st["pad_value"]
    b = torch.from_numpy(np.asarray(boxes, np.float32)).to(dtype)
    s = torch.from_numpy(np.asarray(scores, np.float32)).to(dtype)
    dev = torch.from_numpy(buf.copy()).to(DEV)
    table = None if select is None else torch.tensor(select, dtype=torch.uint8, device=DEV)
    crops = torch.full((N * M * h * w * 3 + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    tensor = None if tensor_dtype is None else torch.full((N * M * 3 * h * w + GUARD,), 7.0, dtype=tensor_dtype, device=DEV)
    counts = torch.full((N + 8,), -7, dtype=torch.int32, device=DEV)
    slots = torch.empty((N, M, _crops.TABLE_INTS), dtype=torch.int32, device=DEV)
    _crops.crop_detections(dev, rows, b.to(DEV), s.to(DEV), torch.from_numpy(np.asarray(labels, np.int64)).to(DEV),
                           torch.from_numpy(np.asarray(count, np.int32)).to(DEV), table, (w, h), M, _crops.FITS[st["fit"]],
                           st["score_thr"], st["expand"], (pad[0] << 16) | (pad[1] << 8) | pad[2], crops, counts, slots,
                           tensor, MEAN, STD)
    got_counts = counts.cpu().numpy()
    assert np.array_equal(dev.cpu().numpy(), buf) and (got_counts[N:] == -7).all()     # the images are only read
    want, want_t = np.full((N, M, h, w, 3), PATTERN, np.uint8), np.full((N, M, 3, h, w), 7.0, np.float32)
    for n, (off, H, W) in enumerate(rows):
        ref, kept = R.crops(buf[off:off + H * W * 3].reshape(H, W, 3), b.float().numpy()[n], s.float().numpy()[n], labels[n], st,
                            select, count[n])
        assert got_counts[n] == len(kept) and slots[n, :len(kept), 0].cpu().tolist() == kept, (n, got_counts[n], kept)
        want[n, :len(kept)], want_t[n, :len(kept)] = ref, R.normalised(ref, MEAN, STD)
    got = crops.cpu().numpy()
    bad = np.argwhere(got[:-GUARD].reshape(want.shape) != want)
    assert len(bad) == 0, f"{len(bad)} bytes differ; first (image, slot, row, column, channel): {bad[:5].tolist()}"
    assert (got[-GUARD:] == PATTERN).all()
    if tensor is not None:   # fp32 as the restatement has it; 16 bits: that value rounded once to nearest even
        expect = torch.cat((torch.from_numpy(want_t).reshape(-1), torch.full((GUARD,), 7.0))).to(tensor_dtype)
        assert torch.equal(tensor.cpu(), expect)
    return got_counts[:N].tolist()


@pytest.mark.parametrize("fit", ["stretch", "pad"])
@pytest.mark.parametrize("name,n,box,size", R.CASES, ids=[c[0] for c in R.CASES])
def test_regions_and_outputs(name, n, box, size, fit):
    """three images at odd byte offsets; the case's box and a copy moved by fractions of a pixel on its image only"""
    buf, rows = cases.buffer(R.SIZES, 21)
    boxes, scores = np.zeros((3, 2, 4), np.float32), np.zeros((3, 2), np.float32)
    boxes[n], scores[n] = box, 0.9
    boxes[n, 1] += (0.25, 0.5, -0.25, 0.0)
    st = dict(size=size, fit=fit, pad_value=(9, 200, 31), max_per_img=3)
    counts = _run(torch.float32, buf, rows, boxes, scores, np.zeros((3, 2), np.int64), [2, 2, 2], st, None, torch.float32)
    assert counts == [2 if i == n else 0 for i in range(3)]


@pytest.mark.parametrize("tensor_dtype", DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_detection_and_tensor_dtypes(dtype, tensor_dtype):
    """the rows of redact_cases.mix (NaN, infinite, outside and zero-width boxes, the score at the threshold, labels
    outside the table, a row beyond count), expand 0.1, five slots for more candidates: the first five in order"""
    buf, rows = cases.buffer(R.SIZES, 22)
    boxes, scores, labels, count = cases.batch()
    st = dict(size=(24, 40), fit="pad", score_thr=cases.THR, expand=0.1, max_per_img=5)
    assert _run(dtype, buf, rows, boxes, scores, labels, count, st, cases.SELECT, tensor_dtype) == [5, 5, 5]


def test_selection():
    buf, rows = cases.buffer(R.SIZES, 23)
    boxes, scores, labels, count = cases.batch()
    st = dict(size=(16, 8), score_thr=cases.THR, max_per_img=16)
    assert _run(torch.float16, buf, rows, boxes, scores, labels, [0, -5, 99], st, cases.SELECT)[:2] == [0, 0]   # 99: clamped to Q
    assert _run(torch.bfloat16, buf, rows, boxes, scores, labels, count, st, [0, 0, 0, 0]) == [0, 0, 0]
    assert _run(torch.float32, buf, rows, boxes, scores, labels, count, dict(st, score_thr=2.0)) == [0, 0, 0]
    assert min(_run(torch.float32, buf, rows, boxes, scores, labels, count, st)) > 6                           # every label
    # the scan's order: Q = 4096, every eleventh row a candidate (373, all rounds and waves) for 256 slots; count 2000: 182
    buf, rows = cases.buffer([(64, 128)], 24)
    boxes, _, labels = cases.crowd(64, 128, 4096, 25)
    scores = np.where(np.arange(4096) % 11 == 3, 0.9, 0.1).astype(np.float32)
    st = dict(size=(8, 8), score_thr=0.5, max_per_img=256)
    assert _run(torch.float32, buf, rows, boxes[None], scores[None], labels[None], [4096], st) == [256]
    assert _run(torch.float32, buf, rows, boxes[None], scores[None], labels[None], [2000], st) == [182]


def test_split_and_operand_checks():
    from codetr import _cabi, hip_ops

    sizes = [(9 + n % 5, 11 + n % 7) for n in range(35)]
    buf, rows = cases.buffer(sizes, 26)
    dev = torch.from_numpy(buf).to(DEV)
    boxes = np.tile(np.asarray([[1.0, 1.0, 8.0, 7.0], [4.5, 3.5, 30.0, 30.0]], np.float32), (35, 1, 1))
    scores = np.full((35, 2), 0.9, np.float32)
    scores[5, 0] = scores[34, 1] = 0.0
    z = torch.zeros

    def dets(N, Q, device=DEV, dtype=torch.float32):
        return hip_ops.Detections(z(N, Q, 4, device=device, dtype=dtype), z(N, Q, device=device, dtype=dtype),
                                  z(N, Q, dtype=torch.int64, device=device), torch.full((N,), Q, dtype=torch.int32, device=device), None)

    d = dets(35, 2)._replace(boxes=torch.from_numpy(boxes).to(DEV), scores=torch.from_numpy(scores).to(DEV))
    st = dict(size=(8, 9), max_per_img=2, tensor=dict(mean=MEAN, std=STD, dtype=torch.float16))
    before = _cabi.CALLS["crop_detections"]
    crops, counts, tensor = hip_ops.crop_detections(dev, rows, d, st)
    assert _cabi.CALLS["crop_detections"] == before + 2 and tensor.shape == (35, 2, 3, 9, 8)        # 32 + 3 images
    for n, (off, H, W) in enumerate(rows):
        ref, kept = R.crops(buf[off:off + H * W * 3].reshape(H, W, 3), boxes[n], scores[n], [0, 0], dict(size=(8, 9), max_per_img=2))
        assert counts[n].item() == len(kept) == (1 if n in (5, 34) else 2) and np.array_equal(crops[n, :len(kept)].cpu().numpy(), ref), n
        assert torch.equal(tensor[n, :len(kept)].cpu(), torch.from_numpy(R.normalised(ref, MEAN, STD)).half()), n
    before, st, one = _cabi.CALLS["crop_detections"], dict(size=(8, 8)), rows[:1]
    for match, args in (("4096", (dev, one, dets(1, 4097), st)), ("GPU", (dev, one, dets(1, 4, device="cpu"), st)),
                        ("GPU", (torch.from_numpy(buf), one, dets(1, 4), st)), ("flat", (dev[::2], one, dets(1, 4), st)),
                        ("outside the buffer", (dev, [(len(buf) - 100, 20, 30)], dets(1, 4), st)),
                        ("select", (dev, one, dets(1, 4), st, z(4, dtype=torch.uint8))),
                        ("dtype", (dev, one, dets(1, 4, dtype=torch.float64), st)), ("len\\(rows\\)", (dev, rows[:2], dets(1, 4), st)),
                        ("size", (dev, one, dets(1, 4), dict(size=(8, 513)))),
                        ("max_per_img", (dev, one, dets(1, 4), dict(st, max_per_img=257)))):
        with pytest.raises(ValueError, match=match):
            hip_ops.crop_detections(*args)
    crops, counts = hip_ops.crop_detections(dev, one, dets(1, 0), st)                  # nothing to do: nothing launched
    assert _cabi.CALLS["crop_detections"] == before and counts.tolist() == [0] and crops.shape == (1, 32, 8, 8, 3)


# ---- the Inferencer ------------------------------------------------------------------------------------------------------
NAMES3 = ["person", "bicycle", "a class name longer than 23 characters"]
SIZES = [(300, 400), (37, 53), (256, 384)]
CROPS = dict(size=(24, 40), classes=["person", 2], score_thr=0.35, expand=0.2, fit="pad", max_per_img=6)
TENSOR = dict(mean=MEAN, std=STD, dtype=torch.bfloat16)


@pytest.mark.parametrize("dtype,batch_size,kw", [(torch.float16, 1, dict()), (torch.bfloat16, 3, dict()),
                                                 (torch.float16, 3, dict(nms_type="config")),
                                                 (torch.bfloat16, 1, dict(nms_type="config"))])
def test_inferencer_returns_the_restatement_of_its_predictions(dtype, batch_size, kw):
    from codetr import _cabi
    from codetr.inferencer import VIS_DOWNLOADS, Inferencer
    from test_tta_gpu import _stub

    images = _images(SIZES, 93)
    originals = [im.copy() for im in images]
    make = lambda **extra: Inferencer(_stub([]), SWIN, dict(classes=NAMES3), score_threshold=0.3, **kw, **extra)  # noqa: E731
    run = dict(device=DEV, dtype=dtype, batch_size=batch_size)
    before, downloads = dict(_cabi.CALLS), VIS_DOWNLOADS["rgb"]
    out = make(crops=dict(CROPS, tensor=TENSOR))(images, **run)
    assert _cabi.CALLS["crop_detections"] - before["crop_detections"] == -(-len(images) // batch_size)   # one per chunk
    assert VIS_DOWNLOADS["rgb"] == downloads                                          # the frame is never downloaded
    before = dict(_cabi.CALLS)
    expect = make()(images, **run)     # crops=None: the counters it moved before, no key
    moved = {k: v - before[k] for k, v in _cabi.CALLS.items() if v != before[k]}
    assert "crop_detections" not in moved
    if batch_size == 3 and not kw:
        assert moved == dict(preprocess_batch=1, postprocess_detections=1)
    assert set(expect) == {"predictions", "visualization"} and all("crop_rows" not in p for p in expect["predictions"])
    _same(out["predictions"], expect["predictions"])
    assert all(np.array_equal(a, b) for a, b in zip(images, originals))              # the caller's arrays are not written
    want = []
    for img, pred in zip(images, out["predictions"]):
        ref, kept = R.crops(img, np.asarray(pred["bboxes"], np.float32).reshape(-1, 4), np.asarray(pred["scores"], np.float32),
                            pred["labels"], {k: v for k, v in CROPS.items() if k != "classes"}, [1, 0, 1])
        assert pred["crop_rows"] == kept
        want.append(ref)
    assert len(out["crops"]) == len(out["crop_tensors"]) == len(images) and sum(len(w) for w in want) > 3
    for got, ten, ref in zip(out["crops"], out["crop_tensors"], want):
        assert got.dtype == np.uint8 and np.array_equal(got, ref) and ten.is_cuda
        assert torch.equal(ten.cpu(), torch.from_numpy(R.normalised(ref, MEAN, STD)).to(torch.bfloat16))
    if batch_size != 3 or kw:
        return
    out2 = make(crops=dict(CROPS, tensor=TENSOR, download=False))(images, **run)      # the tensors only
    assert "crops" not in out2 and all(torch.equal(a, b) for a, b in zip(out2["crop_tensors"], out["crop_tensors"]))
    # with a redaction and a visualiser the crops are still those of the original pixels; the visualisation is not
    out3 = make(crops=CROPS, visualizer=dict(line_width=2), redact=dict(mode="fill", fill=(255, 0, 255), expand=0.5))(
        images, return_vis=True, **run)
    assert all(np.array_equal(a, b) for a, b in zip(out3["crops"], want)) and "crop_tensors" not in out3
    assert any((v == (255, 0, 255)).all(-1).any() for v in out3["visualization"])


def test_track_ids_are_those_of_a_run_without_crops():
    from codetr.inferencer import Inferencer
    from test_tta_gpu import _stub

    images = [_images([(300, 400)], 94)[0].copy() for _ in range(6)]
    kw, run = dict(score_threshold=0.3, tracker={}, track_appearance="color"), dict(device=DEV, dtype=torch.float16, batch_size=3)
    out_a = Inferencer(_stub([]), SWIN, None, crops=dict(size=(16, 8), score_thr=0.5), **kw)(images, **run)
    out_b = Inferencer(_stub([]), SWIN, None, **kw)(images, **run)
    _same(out_a["predictions"], out_b["predictions"])
    assert [p["track_ids"] for p in out_a["predictions"]] == [p["track_ids"] for p in out_b["predictions"]]
    assert all(max(p["crop_rows"], default=-1) < len(p["track_ids"]) for p in out_a["predictions"])
    assert sum(len(c) for c in out_a["crops"]) > 3
