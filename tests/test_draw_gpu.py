"""GPU: the detection drawing -- codetr_draw_detections_* (csrc/draw.hip) bit for bit against the numpy restatement of
its header text (tests/draw_ref.py; integer arithmetic, no tolerance), and `Inferencer(visualizer=...)` end to end with a
stub model: the returned images are the reference drawn from the returned predictions."""
import json
import os

import numpy as np
import pytest
import torch

import draw_ref as R
from test_draw_cpu import read_png
from test_inferencer_batch_gpu import DEV, SWIN, _images, _same

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CLASSES = ["cat", "a", "traffic light", "exactly 23 characters..", "~{|}"]
PALETTE = [(220, 20, 60), (0, 255, 0), (10, 20, 255), (255, 255, 255), (0, 0, 0)]
GUARD = 64


@pytest.fixture(scope="module")
def font():
    from codetr import _cabi

    return _cabi.draw_font()


def _buffer(sizes, seed):
    """images of `sizes` (H, W) in one flat buffer at unaligned offsets, random bytes between and a 64-byte guard
    region behind the last -> (buffer uint8 numpy, rows [(offset, H, W)])"""
    rng = np.random.default_rng(seed)
    rows, offset = [], 1
    for i, (H, W) in enumerate(sizes):
        rows.append((offset, H, W))
        offset += H * W * 3 + (3, 5, 2)[i % 3]
    total = rows[-1][0] + sizes[-1][0] * sizes[-1][1] * 3 + GUARD
    return rng.integers(0, 256, total, dtype=np.uint8), rows


def _run(dtype, buf, rows, boxes, scores, labels, count, font, st, classes=CLASSES, palette=PALETTE):
    """one draw_detections call (as many launches as it needs) -> (the drawn buffer, the reference's), numpy"""
    from codetr import _cabi, hip_ops

    boxes_t = torch.from_numpy(np.asarray(boxes, np.float32)).to(dtype)
    scores_t = torch.from_numpy(np.asarray(scores, np.float32)).to(dtype)
    labels_t = torch.from_numpy(np.asarray(labels, np.int64))
    count_t = torch.from_numpy(np.asarray(count, np.int32))
    dets = hip_ops.Detections(boxes_t.to(DEV), scores_t.to(DEV), labels_t.to(DEV), count_t.to(DEV), None)
    dev = torch.from_numpy(buf.copy()).to(DEV)
    names = hip_ops.draw_names_table(classes).to(DEV)
    colors = torch.tensor(palette, dtype=torch.uint8).to(DEV)
    before = _cabi.CALLS["draw_detections"]
    out = hip_ops.draw_detections(dev, rows, dets, names, colors, st)
    assert out is dev and _cabi.CALLS["draw_detections"] == before + -(-len(rows) // 32)
    expect = R.draw_buffer(buf, rows, boxes_t.float().numpy(), scores_t.float().numpy(), labels_t.numpy(),
                           count_t.numpy(), classes, palette, font, st)
    return dev.cpu().numpy(), expect


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


def _mix(H, W, Q, thr, dtype, rng):
    """Q rows of one image: the cases that decide whether a row is drawn, then heavily overlapping boxes"""
    eps = torch.finfo(dtype).eps
    nan, inf = float("nan"), float("inf")
    boxes = np.zeros((Q, 4), np.float32)
    scores = np.full((Q,), 0.9, np.float32)
    labels = rng.integers(0, len(CLASSES), Q)
    boxes[0] = (-10.3, -5.2, 30.7, 20.1)              # partly outside, negative coordinates
    boxes[1] = (W + 10, H + 10, W + 50, H + 40)       # wholly outside
    boxes[2] = (-100, -100, -50, -60)
    boxes[3] = (40, 10, 39, 20)                       # x2 < x1
    boxes[4] = (10, 10, 10, 10)                       # zero size: one pixel wide
    boxes[5] = (20, 5, 21, 6)                         # two pixels
    boxes[6] = (5, nan, 30, 12)
    boxes[7] = (5, 5, inf, 12)
    boxes[8], labels[8] = (3, 3, 40, 14), -1
    boxes[9], labels[9] = (3, 3, 40, 14), len(CLASSES)
    boxes[10], scores[10] = (2, 2, 50, 12), thr                        # equal: not drawn
    boxes[11], scores[11] = (W - 30, 1, W - 2, 13), thr * (1 + eps)    # just above (exact in the dtype)
    boxes[12], scores[12] = (4, 4, 44, 15), thr * (1 - eps / 2)        # just below
    boxes[13] = (W - 20, H - 9, W + 30, H + 30)       # partly outside at the right and the bottom
    boxes[14] = (-20000, -20000, 20000, 20000)        # clamped: nothing of it is visible
    k = 15
    c = rng.uniform(0, (W, H), (Q - k, 2))
    wh = rng.uniform(2, (W / 1.5, H / 1.5), (Q - k, 2))
    boxes[k:] = np.concatenate((c - wh / 2, c + wh / 2), 1)
    scores[k:] = rng.uniform(thr - 0.05, 1.0, Q - k)
    scores[k] = 1.0
    return boxes, scores, labels


# ---- 1. the kernel against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_reference(dtype, font):
    """three images (97x61, the one-tile 64x16, 130x33) at unaligned offsets, 40 rows each, alpha 0.5: every byte of the
    buffer, the gaps and the guard region included"""
    sizes, Q, thr = [(61, 97), (16, 64), (33, 130)], 40, 0.25
    rng = np.random.default_rng(40)
    buf, rows = _buffer(sizes, 41)
    parts = [_mix(H, W, Q, thr, dtype, rng) for H, W in sizes]
    boxes, scores, labels = (np.stack([p[i] for p in parts]) for i in range(3))
    st = dict(line_width=3, alpha=0.5, score_thr=thr)
    got, expect = _run(dtype, buf, rows, boxes, scores, labels, [Q, Q, Q - 3], font, st)
    _same_bytes(got, expect, rows)
    for (off, H, W), (b, s, l) in zip(rows, parts):
        drawn = [r[0] for r in R.drawn_rows(torch.from_numpy(b).to(dtype).float().numpy(),
                                            torch.from_numpy(s).to(dtype).float().numpy(), l, len(CLASSES), thr)]
        assert 11 in drawn and not set(drawn) & {3, 6, 7, 8, 9, 10, 12} and len(drawn) > 20
    assert not np.array_equal(got, buf)
    assert np.array_equal(got[-GUARD:], buf[-GUARD:]) and got[0] == buf[0]
    # the layers do not commute at alpha 0.5: the same rows in reverse order give another picture
    rev = R.draw_buffer(buf, rows, boxes[:, ::-1], scores[:, ::-1], labels[:, ::-1], [Q, Q, Q], CLASSES, PALETTE, font, st)
    assert not np.array_equal(rev, expect)


@pytest.mark.parametrize("lw", [1, 2, 3])
def test_tile_seams(lw, font):
    """box edges on x = 63 / 64 and y = 15 / 16 and a label grid that spans four tiles of a 130x35 image"""
    buf, rows = _buffer([(35, 130)], 50 + lw)
    boxes = np.asarray([[(63, 2, 64, 30), (10, 15, 120, 16), (64, 16, 100, 30), (0, 0, 63, 15), (48, 8, 125, 33),
                         (62, 14, 65, 17)]], np.float32)
    scores = np.asarray([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]], np.float32)
    labels = np.asarray([[0, 1, 2, 3, 4, 2]])
    st = dict(line_width=lw, alpha=0.5, score_thr=0.3)
    got, expect = _run(torch.float32, buf, rows, boxes, scores, labels, [6], font, st)
    _same_bytes(got, expect, rows)
    ox, oy = 48 + lw, 8 + lw                              # the grid of box 4: "~{|}: 50.0" is 61 font pixels wide
    assert ox < 64 <= ox + 60 and oy < 16 <= oy + 8


def test_list_capacity_and_order(font):
    """count = Q = 4096 overlapping boxes on a 64x32 image (two tiles) at alpha 0.5: every 256-row round appends from
    all four waves to both lists"""
    from codetr import hip_ops

    Q = 4096
    rng = np.random.default_rng(60)
    buf, rows = _buffer([(32, 64)], 61)
    c = rng.uniform(0, (64, 32), (Q, 2))
    wh = rng.uniform(1, (50, 30), (Q, 2))
    boxes = np.concatenate((c - wh / 2, c + wh / 2), 1).astype(np.float32)[None]
    scores = rng.uniform(0.2, 1.0, (1, Q)).astype(np.float32)
    labels = rng.integers(0, len(CLASSES), (1, Q))
    st = dict(line_width=1, alpha=0.5, score_thr=0.3)
    got, expect = _run(torch.float32, buf, rows, boxes, scores, labels, [Q], font, st)
    _same_bytes(got, expect, rows)
    assert len(R.drawn_rows(boxes[0], scores[0], labels[0], len(CLASSES), 0.3)) > 3000
    z = torch.zeros
    big = hip_ops.Detections(z(1, Q + 1, 4, device=DEV), z(1, Q + 1, device=DEV), z(1, Q + 1, dtype=torch.int64, device=DEV),
                             z(1, dtype=torch.int32, device=DEV), None)
    with pytest.raises(ValueError, match="4096"):
        hip_ops.draw_detections(torch.from_numpy(buf).to(DEV), rows, big, hip_ops.draw_names_table(CLASSES).to(DEV),
                                torch.tensor(PALETTE, dtype=torch.uint8, device=DEV))


OPTIONS = {
    "count_zero": (dict(line_width=3, alpha=0.8, score_thr=0.3), [(10, 10, 60, 40)] * 3),
    "no_labels": (dict(line_width=3, alpha=0.8, score_thr=0.3, draw_labels=False), [(10, 10, 60, 40)] * 3),
    "font_scale_2": (dict(line_width=2, alpha=0.8, score_thr=0.3, font_scale=2, text_color=(255, 255, 0)),
                     [(10, 10, 60, 40)] * 3),
    "area_threshold": (dict(line_width=1, alpha=0.8, score_thr=0.3), [(2, 3, 142, 113), (5, 50, 266, 109)]),
    "clipped_label": (dict(line_width=1, alpha=1.0, score_thr=0.3), [(262, 108, 279, 119)]),
}


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_options(option, dtype, font):
    """three images in one buffer, detections on the middle one only: the buffer is the reference's and the other two
    images keep their bytes"""
    st, boxlist = OPTIONS[option]
    sizes = [(20, 30), (120, 280), (45, 70)]
    buf, rows = _buffer(sizes, 70)
    Q = 4
    boxes = np.zeros((3, Q, 4), np.float32)
    scores = np.full((3, Q), 0.875, np.float32)
    labels = np.tile(np.arange(Q) % len(CLASSES), (3, 1))
    for n in range(3):
        boxes[n, :, :] = (1, 1, 18, 15)
    boxes[1, :len(boxlist)] = boxlist
    count = [0, len(boxlist), 0]
    got, expect = _run(dtype, buf, rows, boxes, scores, labels, count, font, st)
    _same_bytes(got, expect, rows)
    for n in (0, 2):
        off, H, W = rows[n]
        assert np.array_equal(got[off:off + H * W * 3], buf[off:off + H * W * 3])
    off, H, W = rows[1]
    img0, img = buf[off:off + H * W * 3].reshape(H, W, 3), got[off:off + H * W * 3].reshape(H, W, 3)
    assert not np.array_equal(img, img0)
    if option == "area_threshold":
        # (140 x 110 = 15400: font pixels of 2 x 2; 261 x 59 = 15399: 1 x 1) -- the grids are 18 and 9 pixels high
        assert (img[4:22, 3] != img0[4:22, 3]).any(-1).all() and (img[22, 3] == img0[22, 3]).all()
        assert (img[51:60, 6] != img0[51:60, 6]).any(-1).all() and (img[60, 6] == img0[60, 6]).all()
    if option == "clipped_label":
        # the grid starts at (263, 109) and runs off the right and the bottom border: no wrap into the next row
        assert tuple(img[109, 263]) == (0, 0, 0) and tuple(img[117, 279]) == (0, 0, 0)      # (grid rows 0 and 8)
        assert np.array_equal(img[110:, 0], img0[110:, 0]) and np.array_equal(img[:108], img0[:108])
    if option == "no_labels":
        assert np.array_equal(img[13:39, 13:59], img0[13:39, 13:59])       # inside the 3-pixel band: untouched


# ---- 2. the Inferencer -----------------------------------------------------------------------------------------------
NAMES3 = ["person", "bicycle", "a class name longer than 23 characters"]
SIZES = [(480, 640), (600, 900), (37, 53), (333, 517), (768, 1152)]
CASES = [
    (torch.float16, 1, dict(nms_type="nms"), "postprocess_detections"),
    (torch.bfloat16, 4, dict(nms_type="config"), "postprocess_softnms"),
    (torch.float16, 4, dict(tta=dict(scales=[(320, 200)], flip=True, nms=dict(type="nms", iou_threshold=0.5),
                                     max_per_img=50)), "tta_merge"),
    (torch.bfloat16, 1, dict(), "postprocess_detections"),
]


@pytest.mark.parametrize("dtype,batch_size,kw,post", CASES)
def test_inferencer_returns_the_reference_drawn_from_its_predictions(dtype, batch_size, kw, post, font, tmp_path):
    from codetr import _cabi
    from codetr.inferencer import Inferencer
    from test_tta_gpu import _stub

    images = _images(SIZES, 80)
    vis = dict(classes=NAMES3, line_width=2, alpha=0.6)
    inf = Inferencer(_stub([]), SWIN, None, score_threshold=0.3, visualizer=vis, **kw)
    plain = Inferencer(_stub([]), SWIN, None, score_threshold=0.3, **kw)
    if kw.get("nms_type") == "nms":
        inf.max_per_img = plain.max_per_img = 10          # the cut travels in the count the kernel is given
    assert inf.soft == (post == "postprocess_softnms")
    chunks = -(-len(images) // batch_size)
    before = dict(_cabi.CALLS)
    out = inf(images, return_vis=True, pred_score_thr=0.4, out_dir=str(tmp_path), no_save_pred=False, device=DEV,
              dtype=dtype, batch_size=batch_size)
    assert _cabi.CALLS["draw_detections"] - before["draw_detections"] == chunks
    assert _cabi.CALLS[post] - before[post] == chunks and _cabi.CALLS["preprocess"] == before["preprocess"]
    before = dict(_cabi.CALLS)
    expect = plain(images, device=DEV, dtype=dtype, batch_size=batch_size)
    assert _cabi.CALLS["draw_detections"] == before["draw_detections"] and expect["visualization"] == []
    _same(out["predictions"], expect["predictions"])
    assert len(out["visualization"]) == len(images) and inf.num_visualized_imgs == inf.num_predicted_imgs == 5
    palette = inf.visualizer["palette"]
    st = dict(line_width=2, alpha=0.6, score_thr=0.4)
    total = 0
    for i, (img, pred, drawn) in enumerate(zip(images, out["predictions"], out["visualization"])):
        assert drawn.dtype == np.uint8 and drawn.shape == img.shape
        ref = R.draw(img, np.asarray(pred["bboxes"], np.float32).reshape(-1, 4), np.asarray(pred["scores"], np.float32),
                     pred["labels"], NAMES3, palette, font, st)
        assert np.array_equal(drawn, ref), i
        total += int((drawn != img).any(-1).sum())
        assert np.array_equal(read_png(os.path.join(tmp_path, "vis", "%08d.png" % i)), drawn)
        assert json.load(open(os.path.join(tmp_path, "preds", f"{i}.json"))) == pred
        if kw.get("nms_type") == "nms":
            assert len(pred["labels"]) <= 10
    assert total > 1000 and sum(len(p["labels"]) for p in out["predictions"]) > 10
    assert sorted(os.listdir(tmp_path / "vis")) == ["%08d.png" % i for i in range(5)]


def test_inferencer_without_drawing_launches_nothing(tmp_path):
    from codetr import _cabi
    from codetr.inferencer import Inferencer
    from test_tta_gpu import _stub

    images = _images(SIZES[:3], 81)
    inf = Inferencer(_stub([]), SWIN, None, score_threshold=0.3, visualizer=dict(classes=NAMES3))
    before = _cabi.CALLS["draw_detections"]
    out = inf(images, return_vis=True, draw_pred=False, device=DEV, dtype=torch.float16, batch_size=2)
    assert _cabi.CALLS["draw_detections"] == before
    assert all(np.array_equal(a, b) and a is not b for a, b in zip(out["visualization"], images))
    # neither return_vis nor an out_dir: the visualizer is idle; no_save_vis keeps the pictures off the disk
    out = inf(images, device=DEV, dtype=torch.float16, batch_size=2)
    assert _cabi.CALLS["draw_detections"] == before and out["visualization"] == []
    out = inf(images, out_dir=str(tmp_path), no_save_vis=True, no_save_pred=False, device=DEV, dtype=torch.float16)
    assert _cabi.CALLS["draw_detections"] == before and os.listdir(tmp_path) == ["preds"]
    assert sorted(os.listdir(tmp_path / "preds")) == ["6.json", "7.json", "8.json"]
    # the tables go up once per device
    inf(images, return_vis=True, device=DEV, dtype=torch.float16, batch_size=2)
    tables = dict(inf._vis_tables)
    inf(images, return_vis=True, device=DEV, dtype=torch.float16, batch_size=3)
    assert _cabi.CALLS["draw_detections"] == before + 3 and len(tables) == 1
    assert all(inf._vis_tables[k][0] is tables[k][0] for k in tables)
