"""GPU: the redaction -- codetr_redact_detections_* (csrc/redact.hip) byte for byte against the numpy restatement of its
header text (tests/redact_ref.py; integer arithmetic, no tolerance), and `Inferencer(redact=...)` end to end with a stub
model: the returned images are the restatement applied to the inputs with the returned predictions."""
import itertools
import os

import numpy as np
import pytest
import torch

import draw_ref
import jpeg_ref
import redact_cases as cases
import redact_ref as R
from test_inferencer_batch_gpu import DEV, SWIN, _images, _same

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MODES, SHAPES = ("pixelate", "blur", "fill"), ("box", "ellipse")


def _dets(dtype, boxes, scores, labels, count):
    from codetr import hip_ops

    b = torch.from_numpy(np.asarray(boxes, np.float32)).to(dtype)
    s = torch.from_numpy(np.asarray(scores, np.float32)).to(dtype)
    l = torch.from_numpy(np.asarray(labels, np.int64))
    c = torch.from_numpy(np.asarray(count, np.int32))
    return hip_ops.Detections(b.to(DEV), s.to(DEV), l.to(DEV), c.to(DEV), None), b.float().numpy(), s.float().numpy()


def _run(dtype, buf, rows, boxes, scores, labels, count, st, select=None):
    """one redact_detections call -> (the redacted buffer, the restatement's), numpy"""
    from codetr import _cabi, hip_ops

    dets, b, s = _dets(dtype, boxes, scores, labels, count)
    dev = torch.from_numpy(buf.copy()).to(DEV)
    table = None if select is None else torch.tensor(select, dtype=torch.uint8, device=DEV)
    before = _cabi.CALLS["redact_detections"]
    out = hip_ops.redact_detections(dev, rows, dets, st, table)
    assert out is dev and _cabi.CALLS["redact_detections"] == before + -(-len(rows) // 32)
    return dev.cpu().numpy(), R.redact_buffer(buf, rows, b, s, labels, count, st, select)


def _same_bytes(got, expect, rows):
    if not np.array_equal(got, expect):
        bad = np.flatnonzero(got != expect)
        where = []
        for i in bad[:5]:
            n = max(k for k, r in enumerate(rows) if r[0] <= i) if i >= rows[0][0] else -1
            off, H, W = rows[n]
            p = (int(i) - off) // 3
            where.append((n, p % W, p // W, int(got[i]), int(expect[i])))
        raise AssertionError(f"{len(bad)} bytes differ; first (image, x, y, got, expected): {where}")


# ---- 1. the kernel against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,shape", list(itertools.product(MODES, SHAPES)))
def test_modes_shapes_and_dtypes(mode, shape, dtype):
    """three images (70x131, 5x7, 64x128) at odd byte offsets, the sixteen rows of redact_cases.mix each: every byte of
    the buffer, the gaps and the guard region included"""
    buf, rows = cases.buffer(cases.SIZES, 11)
    boxes, scores, labels, count = cases.batch()
    st = dict(mode=mode, shape=shape, score_thr=cases.THR, fill=(9, 200, 31))
    got, expect = _run(dtype, buf, rows, boxes, scores, labels, count, st, cases.SELECT)
    _same_bytes(got, expect, rows)
    assert not np.array_equal(got, buf)
    assert np.array_equal(got[-cases.GUARD:], buf[-cases.GUARD:]) and got[0] == buf[0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cell,expand", [(4, 0.0), (16, 0.1), (64, 1.0), (4, 1.0), (64, 0.0), (8, 0.1), (32, 0.1)])
def test_cells_and_expand(mode, cell, expand):
    buf, rows = cases.buffer(cases.SIZES, 12)
    boxes, scores, labels, count = cases.batch()
    st = dict(mode=mode, shape="ellipse" if cell == 16 else "box", cell=cell, expand=expand, score_thr=cases.THR)
    got, expect = _run(torch.float16, buf, rows, boxes, scores, labels, count, st)      # no table: every label
    _same_bytes(got, expect, rows)
    assert not np.array_equal(got, buf)


@pytest.mark.parametrize("mode", MODES)
def test_count_zero_and_no_selected_row_leave_the_buffer(mode):
    buf, rows = cases.buffer(cases.SIZES, 13)
    boxes, scores, labels, count = cases.batch()
    st = dict(mode=mode, score_thr=cases.THR)
    got, expect = _run(torch.bfloat16, buf, rows, boxes, scores, labels, [0, 0, 0], st, cases.SELECT)
    assert np.array_equal(got, buf) and np.array_equal(expect, buf)
    got, expect = _run(torch.bfloat16, buf, rows, boxes, scores, labels, [0, -5, 99], st, [0, 0, 0, 0])
    assert np.array_equal(got, buf) and np.array_equal(expect, buf)
    got, expect = _run(torch.float32, buf, rows, boxes, scores, labels, count, dict(st, score_thr=2.0))
    assert np.array_equal(got, buf) and np.array_equal(expect, buf)
    # count above Q is clamped to Q: the row beyond count joins
    got, expect = _run(torch.float32, buf, rows, boxes, scores, labels, [99, 99, 99], st, cases.SELECT)
    _same_bytes(got, expect, rows)


@pytest.mark.parametrize("mode,shape", [("blur", "ellipse"), ("pixelate", "box")])
def test_list_capacity(mode, shape):
    """count = Q = 4096 random overlapping boxes on a 64x128 image (two tiles): sixteen gather rounds, most rows reach
    both tiles"""
    Q = 4096
    buf, rows = cases.buffer([(64, 128)], 14)
    boxes, scores, labels = cases.crowd(64, 128, Q, 15)
    st = dict(mode=mode, shape=shape, cell=8, score_thr=0.3)
    assert len(R.selected_rows(boxes, scores, labels, Q, 0.3)) >= 3000
    regs = [R.region(boxes[j], st.get("expand", 0.1)) for j in R.selected_rows(boxes, scores, labels, Q, 0.3)]
    assert sum(r is not None for r in regs) >= 3000
    got, expect = _run(torch.float32, buf, rows, boxes[None], scores[None], labels[None], [Q], st)
    _same_bytes(got, expect, rows)
    off, H, W = rows[0]
    changed = (got[off:off + H * W * 3] != buf[off:off + H * W * 3]).reshape(H, W, 3).any(-1)
    assert changed.mean() > 0.5


@pytest.mark.parametrize("mode", MODES)
def test_seams(mode):
    """regions (expand 0) that end one pixel either side of the tile edge at 64 and of the cell edges at 16 and 48, for x
    and for y, on a 130 x 135 image (three tiles each way, the last a sliver)"""
    buf, rows = cases.buffer([(130, 135)], 16)
    edges = []
    for e in (16, 48, 64, 128):
        edges += [(3.0, 5.0, e - 1.0, 9.0), (3.0, 11.0, float(e), 15.0), (3.0, 17.0, e + 1.0, 21.0),       # x2 around e
                  (e - 1.0, 23.0, 133.0, 27.0), (float(e), 29.0, 133.0, 33.0), (e + 1.0, 35.0, 133.0, 39.0),  # x1
                  (70.0, 2.0, 74.0, e - 1.0), (76.0, 2.0, 80.0, float(e)), (82.0, 2.0, 86.0, e + 1.0),        # y2
                  (88.0, e - 1.0, 92.0, 129.0), (94.0, float(e), 98.0, 129.0), (100.0, e + 1.0, 104.0, 129.0)]
    boxes = np.asarray(edges, np.float32)[None]
    Q = boxes.shape[1]
    scores, labels = np.full((1, Q), 0.9, np.float32), np.zeros((1, Q), np.int64)
    for shape in SHAPES:
        st = dict(mode=mode, shape=shape, cell=16, expand=0.0)
        got, expect = _run(torch.float32, buf, rows, boxes, scores, labels, [Q], st)
        _same_bytes(got, expect, rows)
    off, H, W = rows[0]
    img0, img = buf[off:off + H * W * 3].reshape(H, W, 3), got[off:off + H * W * 3].reshape(H, W, 3)
    assert np.array_equal(img[0:2], img0[0:2]) and np.array_equal(img[:, 134], img0[:, 134])


def test_more_than_32_images_split():
    sizes = [(9 + n % 5, 11 + n % 7) for n in range(35)]
    buf, rows = cases.buffer(sizes, 17)
    boxes = np.tile(np.asarray([[1.0, 1.0, 8.0, 7.0], [4.5, 3.5, 30.0, 30.0]], np.float32), (35, 1, 1))
    scores, labels = np.full((35, 2), 0.9, np.float32), np.zeros((35, 2), np.int64)
    for mode in MODES:
        got, expect = _run(torch.float16, buf, rows, boxes, scores, labels, [2] * 35, dict(mode=mode, cell=4))
        _same_bytes(got, expect, rows)


def test_operand_checks():
    from codetr import _cabi, hip_ops

    buf, rows = cases.buffer([(20, 30)], 18)
    dev = torch.from_numpy(buf).to(DEV)
    z = torch.zeros

    def dets(Q, device=DEV, dtype=torch.float32):
        return hip_ops.Detections(z(1, Q, 4, device=device, dtype=dtype), z(1, Q, device=device, dtype=dtype),
                                  z(1, Q, dtype=torch.int64, device=device), z(1, dtype=torch.int32, device=device), None)

    before = _cabi.CALLS["redact_detections"]
    with pytest.raises(ValueError, match="4096"):
        hip_ops.redact_detections(dev, rows, dets(4097))
    with pytest.raises(ValueError, match="GPU"):
        hip_ops.redact_detections(dev, rows, dets(4, device="cpu"))
    with pytest.raises(ValueError, match="GPU"):
        hip_ops.redact_detections(torch.from_numpy(buf), rows, dets(4))
    with pytest.raises(ValueError, match="flat"):
        hip_ops.redact_detections(dev[:1800].view(20, 90), rows, dets(4))
    with pytest.raises(ValueError, match="flat"):
        hip_ops.redact_detections(dev[::2], rows, dets(4))
    with pytest.raises(ValueError, match="outside the buffer"):
        hip_ops.redact_detections(dev, [(len(buf) - 100, 20, 30)], dets(4))
    with pytest.raises(ValueError, match="outside the buffer"):
        hip_ops.redact_detections(dev, [(-1, 20, 30)], dets(4))
    with pytest.raises(ValueError, match="select"):
        hip_ops.redact_detections(dev, rows, dets(4), None, z(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="select"):
        hip_ops.redact_detections(dev, rows, dets(4), None, z(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="dtype"):
        hip_ops.redact_detections(dev, rows, dets(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="len\\(rows\\)"):
        hip_ops.redact_detections(dev, rows + rows, dets(4))
    with pytest.raises(ValueError, match="cell"):
        hip_ops.redact_detections(dev, rows, dets(4), dict(cell=12))
    assert _cabi.CALLS["redact_detections"] == before
    # nothing to do: nothing launched
    assert hip_ops.redact_detections(dev, rows, dets(0)) is dev and hip_ops.redact_detections(dev, [], hip_ops.Detections(
        z(0, 4, 4, device=DEV), z(0, 4, device=DEV), z(0, 4, dtype=torch.int64, device=DEV), z(0, dtype=torch.int32, device=DEV),
        None)) is dev
    assert _cabi.CALLS["redact_detections"] == before and np.array_equal(dev.cpu().numpy(), buf)


# ---- 2. the Inferencer -----------------------------------------------------------------------------------------------
NAMES3 = ["person", "bicycle", "a class name longer than 23 characters"]
SIZES = [(300, 400), (37, 53), (256, 384)]
CASES = [(torch.float16, 1, dict()), (torch.bfloat16, 3, dict()), (torch.float16, 3, dict(nms_type="config")),
         (torch.bfloat16, 1, dict(nms_type="config"))]
REDACT = dict(mode="blur", classes=["person", 2], score_thr=0.35, expand=0.2, shape="ellipse", cell=8)


def _expected(images, preds, redact, select):
    out = []
    for img, pred in zip(images, preds):
        red, rows = R.redact(img, np.asarray(pred["bboxes"], np.float32).reshape(-1, 4), np.asarray(pred["scores"], np.float32),
                             pred["labels"], {k: v for k, v in redact.items() if k != "classes"}, select)
        assert pred["redacted"] == rows
        out.append(red)
    return out


@pytest.mark.parametrize("dtype,batch_size,kw", CASES)
def test_inferencer_returns_the_restatement_of_its_predictions(dtype, batch_size, kw, tmp_path):
    from codetr import _cabi
    from codetr.inferencer import Inferencer
    from test_tta_gpu import _stub

    images = _images(SIZES, 90)
    originals = [im.copy() for im in images]
    meta = dict(classes=NAMES3)
    inf = Inferencer(_stub([]), SWIN, meta, score_threshold=0.3, redact=REDACT, **kw)
    plain = Inferencer(_stub([]), SWIN, meta, score_threshold=0.3, **kw)
    if "nms_type" not in kw:
        inf.max_per_img = plain.max_per_img = 10          # the cut travels in the count the kernel is given
    chunks = -(-len(images) // batch_size)
    before = dict(_cabi.CALLS)
    out = inf(images, return_vis=True, device=DEV, dtype=dtype, batch_size=batch_size)
    assert _cabi.CALLS["redact_detections"] - before["redact_detections"] == chunks
    assert _cabi.CALLS["draw_detections"] == before["draw_detections"]
    expect = plain(images, device=DEV, dtype=dtype, batch_size=batch_size)
    assert all("redacted" not in p for p in expect["predictions"])
    _same(out["predictions"], expect["predictions"])
    assert all(np.array_equal(a, b) for a, b in zip(images, originals))              # the caller's arrays are not written
    redacted = _expected(images, out["predictions"], REDACT, [1, 0, 1])
    assert len(out["visualization"]) == len(images)
    for i, (got, ref, img) in enumerate(zip(out["visualization"], redacted, images)):
        assert np.array_equal(got, ref), i
    assert sum((r != im).any(-1).sum() for r, im in zip(redacted, images)) > 100
    assert sum(len(p["redacted"]) for p in out["predictions"]) > 3
    if "nms_type" not in kw:
        assert all(len(p["labels"]) <= 10 for p in out["predictions"])

    # with a visualiser the outlines and labels lie over the redacted pixels; draw_pred=False leaves them off
    vis = dict(line_width=2, alpha=0.6)
    both = Inferencer(_stub([]), SWIN, meta, score_threshold=0.3, redact=REDACT, visualizer=vis, vis_format="jpeg", **kw)
    both.max_per_img = inf.max_per_img
    font = _cabi.draw_font()
    out2 = both(images, return_vis=True, pred_score_thr=0.4, out_dir=str(tmp_path), device=DEV, dtype=dtype,
                batch_size=batch_size)
    st = dict(line_width=2, alpha=0.6, score_thr=0.4)
    for i, (got, red, pred) in enumerate(zip(out2["visualization"], redacted, out2["predictions"])):
        ref = draw_ref.draw(red, np.asarray(pred["bboxes"], np.float32).reshape(-1, 4), np.asarray(pred["scores"], np.float32),
                            pred["labels"], NAMES3, both.visualizer["palette"], font, st)
        assert np.array_equal(got, ref), i
        assert open(os.path.join(tmp_path, "vis", "%08d.jpg" % i), "rb").read() == jpeg_ref.encode(ref, 90, "420")
    out3 = both(images, return_vis=True, draw_pred=False, device=DEV, dtype=dtype, batch_size=batch_size)
    assert all(np.array_equal(a, b) for a, b in zip(out3["visualization"], redacted))
    # neither return_vis nor an out_dir: no image leaves the call, nothing is launched, the key is there
    before = dict(_cabi.CALLS)
    out4 = inf(images, device=DEV, dtype=dtype, batch_size=batch_size)
    assert _cabi.CALLS["redact_detections"] == before["redact_detections"] and out4["visualization"] == []
    assert [p["redacted"] for p in out4["predictions"]] == [p["redacted"] for p in out["predictions"]]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_track_ids_are_those_of_a_run_without_redaction(dtype):
    """the appearance descriptors read the pixels before the redaction writes them"""
    from codetr.inferencer import Inferencer
    from test_tta_gpu import _stub

    images = [_images([(300, 400)], 91)[0].copy() for _ in range(6)]          # a still scene: the tracks are confirmed
    kw = dict(score_threshold=0.3, tracker={}, track_appearance="color")
    a = Inferencer(_stub([]), SWIN, None, redact=dict(mode="fill", fill=(255, 0, 255), expand=0.5), **kw)
    b = Inferencer(_stub([]), SWIN, None, **kw)
    out_a = a(images, return_vis=True, device=DEV, dtype=dtype, batch_size=3)
    out_b = b(images, device=DEV, dtype=dtype, batch_size=3)
    _same(out_a["predictions"], out_b["predictions"])
    assert [p["track_ids"] for p in out_a["predictions"]] == [p["track_ids"] for p in out_b["predictions"]]
    assert any(i > 0 for p in out_a["predictions"] for i in p["track_ids"])
    assert sum((v != im).any(-1).sum() for v, im in zip(out_a["visualization"], images)) > 100


def test_default_is_unchanged():
    """redact=None: the launches of a call are those of before (no new counter moves), no key, and return_vis without a
    visualiser still raises"""
    from codetr import _cabi
    from codetr.inferencer import Inferencer
    from test_tta_gpu import _stub

    images = _images(SIZES, 92)
    inf = Inferencer(_stub([]), SWIN, None, score_threshold=0.3, visualizer=dict(classes=NAMES3))
    assert inf.redact is None
    before = dict(_cabi.CALLS)
    out = inf(images, return_vis=True, device=DEV, dtype=torch.float16, batch_size=2)
    moved = {k: v - before[k] for k, v in _cabi.CALLS.items() if v != before[k]}
    assert moved == dict(preprocess_batch=2, postprocess_detections=2, draw_detections=2)
    assert all(set(p) == {"labels", "scores", "bboxes"} for p in out["predictions"])
    bare = Inferencer(_stub([]), SWIN, None, score_threshold=0.3)
    with pytest.raises(NotImplementedError):
        bare(images, return_vis=True, device=DEV, dtype=torch.float16)
    before = dict(_cabi.CALLS)
    bare(images, device=DEV, dtype=torch.float16, batch_size=2)
    assert {k: v - before[k] for k, v in _cabi.CALLS.items() if v != before[k]} == dict(preprocess_batch=2,
                                                                                         postprocess_detections=2)
