"""CPU: the detection drawing's reference (tests/draw_ref.py) against hand-computed answers, the library's 5x7 font
through its host-only accessor, and the host side of `Inferencer(visualizer=...)`: settings, class-name and palette
tables, the PNG writer and the prediction files.  No GPU call."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

import draw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIN = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")


@pytest.fixture(scope="module")
def font():
    from codetr import _cabi

    return _cabi.draw_font()


def _one_box(box, lw, alpha, fill=100, color=(10, 20, 30), H=10, W=12):
    img = np.full((H, W, 3), fill, np.uint8)
    out = R.draw(img, [box], [0.9], [0], ["x"], [color], bytes(665),
                 dict(line_width=lw, alpha=alpha, score_thr=0.3, draw_labels=False))
    changed = {(x, y) for y, x in zip(*np.nonzero((out != img).any(-1)))}
    return out, changed


# ---- 1. the reference against hand-computed answers ---------------------------------------------------------------
def test_edge_pixels_of_a_one_pixel_line():
    """12x10 image, box (2, 3, 8, 7), lw 1 (a = b = 0), alpha 1: the perimeter of [2, 8] x [3, 7], nothing else"""
    out, changed = _one_box((2.0, 3.0, 8.0, 7.0), 1, 1.0)
    expect = {(x, y) for x in range(2, 9) for y in (3, 7)} | {(x, y) for x in (2, 8) for y in range(3, 8)}
    assert changed == expect and len(expect) == 20
    assert all(tuple(out[y, x]) == (10, 20, 30) for x, y in expect)          # A = 256: the colour itself


def test_rounding_and_clamping_of_coordinates():
    """floor(x + 0.5): 2.5 -> 3, 2.49 -> 2, -0.5 -> 0, -0.51 -> -1; clamped to [-16384, 16383] first"""
    assert [R.pixel_coord(v) for v in (2.5, 2.49, -0.5, -0.51, 1e9, -1e9, 16383.4)] == [3, 2, 0, -1, 16383, -16384, 16383]
    _, changed = _one_box((1.5, 2.49, 8.49, 6.5), 1, 1.0)
    assert changed == _one_box((2.0, 2.0, 8.0, 7.0), 1, 1.0)[1]


def test_three_pixel_line_blends_at_alpha_point_eight():
    """lw 3 (a = b = 1): band [1, 9] x [2, 8] minus [4, 6] x [5, 5]; A = int(0.8 * 256 + 0.5) = 205"""
    assert R.alpha_weight(0.8) == 205
    out, changed = _one_box((2.0, 3.0, 8.0, 7.0), 3, 0.8, fill=100, color=(10, 20, 255))
    expect = {(x, y) for x in range(1, 10) for y in range(2, 9)} - {(4, 5), (5, 5), (6, 5)}
    assert changed == expect
    assert tuple(out[3, 2]) == ((100 * 51 + 10 * 205 + 128) >> 8, (100 * 51 + 20 * 205 + 128) >> 8,
                                (100 * 51 + 255 * 205 + 128) >> 8) == (28, 36, 224)
    assert tuple(out[5, 5]) == (100, 100, 100)


def test_two_pixel_line_grows_outwards():
    """lw 2: a = 1, b = 0 -- the extra pixel is on the outside: columns x1 - 1 and x1, x2 and x2 + 1"""
    _, changed = _one_box((3.0, 2.0, 8.0, 7.0), 2, 1.0)
    row = sorted(x for x, y in changed if y == 4)
    assert row == [2, 3, 8, 9]
    col = sorted(y for x, y in changed if x == 5)
    assert col == [1, 2, 7, 8]


def test_an_empty_inner_rectangle_fills_the_box():
    _, changed = _one_box((3.0, 3.0, 4.0, 4.0), 3, 1.0)            # inner [5, 2]: empty
    assert changed == {(x, y) for x in range(2, 6) for y in range(2, 6)}
    _, changed = _one_box((3.0, 3.0, 3.0, 3.0), 1, 1.0)            # a zero-size box is one pixel
    assert changed == {(3, 3)}
    _, changed = _one_box((3.0, 3.0, 2.0, 5.0), 1, 1.0)            # x2 < x1: not drawn
    assert changed == set()


def test_the_drawn_set():
    nan, inf = float("nan"), float("inf")
    boxes = [(1, 1, 5, 5)] * 6 + [(1, nan, 5, 5), (1, 1, inf, 5), (5, 1, 4, 5), (1, 5, 5, 4.4)]
    scores = [0.3, np.nextafter(np.float32(0.3), np.float32(1)), np.nextafter(np.float32(0.3), np.float32(0)), nan, 0.9,
              0.9, 0.9, 0.9, 0.9, 0.9]
    labels = [0, 0, 0, 0, -1, 3, 0, 0, 0, 0]
    rows = R.drawn_rows(np.asarray(boxes, np.float32), np.asarray(scores, np.float32), labels, 3, 0.3)
    assert [r[0] for r in rows] == [1]       # strictly above the threshold, label in range, finite, ordered corners


def test_score_text():
    assert [R.score_text(s) for s in (0.873, 0.05, 1.0, 0.99996, 0.0004)] == ["87.3", "5.0", "100.0", "100.0", "0.0"]
    assert R.score_text(0.99949) == "99.9" and R.score_text(7.0) == "100.0" and R.score_text(-0.2) == "0.0"
    assert R.score_text(float("inf")) == "100.0"


def test_label_grid_known_answer(font):
    """'!' is one column of ink (glyph column 2, rows 0..4 and 6): with lw 1 and the box at (2, 1) the grid starts at
    (3, 2); the text "!: 5.0" has 6 characters -> 37 x 9 font pixels; the labels go over the edges"""
    img = np.full((20, 48, 3), 200, np.uint8)
    st = dict(line_width=1, alpha=0.5, score_thr=0.0, text_color=(1, 2, 3))
    out = R.draw(img, [(2.0, 1.0, 30.0, 15.0), (5.0, -30.0, 5.0, 19.0)], [0.05, 0.05], [0, 0], ["!"], [(0, 0, 255)], font, st)
    ink = {(3 + 1 + 2, 2 + 1 + r) for r in (0, 1, 2, 3, 4, 6)}
    for x, y in ink:
        assert tuple(out[y, x]) == (1, 2, 3)
    assert tuple(out[2 + 6, 3 + 3]) == (100, 100, 100)                    # the gap of '!': 200 blended with black at 128
    assert tuple(out[2, 3]) == (100, 100, 100) and tuple(out[10, 39]) == (100, 100, 100)   # grid corners (37 x 9)
    assert tuple(out[11, 20]) == (200, 200, 200) and tuple(out[5, 40]) == (200, 200, 200)  # just outside it
    # the second box (its own label is above the image) has its edge in column 5: drawn before the labels, so inside
    # the first box's grid it is darkened once more
    edge = (200 * 128 + 255 * 128 + 128) >> 8
    assert tuple(out[18, 5]) == ((200 * 128 + 128) >> 8, (200 * 128 + 128) >> 8, edge)
    assert tuple(out[5, 5]) == ((100 * 128 + 128) >> 8, (100 * 128 + 128) >> 8, (edge * 128 + 128) >> 8)
    # a box of area >= 15400 doubles the font pixel
    big = R.draw(np.zeros((200, 200, 3), np.uint8), [(0.0, 0.0, 140.0, 110.0)], [0.5], [0], ["!"], [(0, 0, 0)], font, st)
    assert tuple(big[1 + 2, 1 + 2 * 3]) == (1, 2, 3) and tuple(big[1 + 3, 1 + 2 * 3 + 1]) == (1, 2, 3)


def test_labels_are_clipped_not_shifted(font):
    img = np.full((8, 10, 3), 255, np.uint8)
    out = R.draw(img, [(6.0, 4.0, 9.0, 7.0)], [0.5], [0], ["W"], [(0, 0, 0)], font, dict(line_width=1, alpha=1.0))
    assert tuple(out[5, 7]) == (0, 0, 0) and tuple(out[7, 9]) in ((0, 0, 0), (200, 200, 200))
    assert (out[:4] == 255).all() and (out[:, :6] == 255).all()


# ---- 2. the font ---------------------------------------------------------------------------------------------------
def test_font_from_the_library(font):
    assert len(font) == 665
    glyphs = np.frombuffer(font, np.uint8).reshape(95, 7)
    assert not glyphs[0].any()                                            # space
    assert all(glyphs[i].any() for i in range(1, 95))
    assert not (glyphs & 0xE0).any()                                      # the low 5 bits only
    assert len({bytes(g) for g in glyphs}) == 95                          # pairwise distinct
    for d in "0123456789":
        g = glyphs[ord(d) - 32]
        assert g[0] and g[6], d
    from codetr import _cabi

    assert _cabi.load().codetr_draw_font(None) == -1


# ---- 3. settings ---------------------------------------------------------------------------------------------------
def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    return Inferencer(None, kw.pop("cfg", SWIN), kw.pop("dataset_meta", None), **kw)


def test_without_a_visualizer_return_vis_still_raises():
    inf = _inferencer()
    assert inf.visualizer is None
    img = np.zeros((4, 4, 3), np.uint8)
    for kw in (dict(return_vis=True), dict(show=True), dict(return_datasamples=True)):
        with pytest.raises(NotImplementedError):
            inf([img], **kw)
    for kw in (dict(show=True), dict(return_datasamples=True)):
        with pytest.raises(NotImplementedError):
            _inferencer(visualizer={})([img], **kw)


def test_visualizer_validation():
    for bad in (dict(line_width=0), dict(line_width=16), dict(line_width=2.5), dict(alpha=1.5), dict(alpha=-0.1),
                dict(font_scale=5), dict(text_color=(1, 2)), dict(text_color=(1, 2, 300)), dict(colour=1),
                dict(score_thr=0.5), dict(palette=[(1, 2, 3)]), dict(classes=[])):
        with pytest.raises(ValueError):
            _inferencer(visualizer=bad)
    with pytest.raises(ValueError):
        _inferencer(visualizer="mmdet")
    v = _inferencer(visualizer={}).visualizer
    assert v["style"] == dict(line_width=3, alpha=0.8, score_thr=0.3, text_color=(200, 200, 200), font_scale=1,
                              draw_labels=True)
    assert v["classes"] == [str(i) for i in range(80)] and len(v["palette"]) == 80
    v = _inferencer(visualizer=dict(line_width=5, alpha=0.25, draw_labels=False, font_scale=2)).visualizer["style"]
    assert (v["line_width"], v["alpha"], v["draw_labels"], v["font_scale"]) == (5, 0.25, False, 2)


def test_visualizer_from_the_config(tmp_path):
    with pytest.raises(ValueError, match="visualizer"):
        _inferencer(visualizer="config")                                  # the shipped configs have no such entry
    cfg = tmp_path / "with_visualizer.py"
    cfg.write_text(f"_base_ = {SWIN!r}\nvisualizer = dict(type='DetLocalVisualizer', name='visualizer', line_width=2, "
                   "alpha=0.5, text_color=(255, 255, 0), vis_backends=[dict(type='LocalVisBackend')])\n")
    st = _inferencer(cfg=str(cfg), visualizer="config").visualizer["style"]
    assert (st["line_width"], st["alpha"], st["text_color"], st["font_scale"]) == (2, 0.5, (255, 255, 0), 1)


def test_class_names_and_palette_sources():
    from codetr import hip_ops
    from codetr.inferencer import generated_palette

    meta = dict(classes=("person", "bicycle"), palette=[(220, 20, 60), (119, 11, 32)])
    v = _inferencer(visualizer={}, dataset_meta=meta).visualizer
    assert v["classes"] == ["person", "bicycle"] and v["palette"] == [(220, 20, 60), (119, 11, 32)]
    v = _inferencer(visualizer=dict(classes=["a", "b", "c"], palette="coco"), dataset_meta=meta).visualizer
    assert v["classes"] == ["a", "b", "c"] and v["palette"] == generated_palette(3)
    assert v["colors"].tolist() == [list(c) for c in generated_palette(3)]
    # determinism and spread of the generated table
    p = generated_palette(80)
    assert p == generated_palette(80) and p[:3] == generated_palette(3) and len(set(p)) == 80
    assert all(0 <= c <= 255 for t in p for c in t) and p[0] == (255, 64, 64)
    # truncation to 23 characters, '?' for anything outside ASCII 32..126
    long = "a very long class name indeed"
    t = hip_ops.draw_names_table(["cat", long, "café\tx", ""])
    assert tuple(t.shape) == (4, 24) and t[:, 0].tolist() == [3, 23, 6, 0]
    assert bytes(t[1, 1:].tolist()) == long[:23].encode() and bytes(t[2, 1:7].tolist()) == b"caf??x"
    assert bytes(t[0, 1:].tolist()) == b"cat" + bytes(20)
    assert np.array_equal(t.numpy(), R.names_table(["cat", long, "café\tx", ""]))


def test_draw_detections_rejects_cpu_tensors_and_bad_styles():
    import torch

    from codetr import hip_ops

    z = torch.zeros
    dets = hip_ops.Detections(z(1, 2, 4), z(1, 2), z(1, 2, dtype=torch.int64), z(1, dtype=torch.int32), None)
    with pytest.raises(ValueError):
        hip_ops.draw_detections(z(48, dtype=torch.uint8), [(0, 4, 4)], dets, z(1, 24, dtype=torch.uint8),
                                z(1, 3, dtype=torch.uint8))
    for bad in (dict(line_width=0), dict(alpha=1.5), dict(font_scale=0), dict(thickness=1), dict(score_thr=float("nan"))):
        with pytest.raises(ValueError):
            hip_ops.draw_style(bad)


# ---- 4. files ------------------------------------------------------------------------------------------------------
def read_png(path):
    """the decoder of the writer's subset: 8-bit RGB, filter 0 on every row"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, shape = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", body)
            assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
            shape = (H, W)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert tag == b"IEND"
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(shape[0], shape[1], 3)


def test_png_writer_round_trips(tmp_path):
    from codetr.inferencer import write_png

    rng = np.random.default_rng(0)
    for H, W in ((1, 1), (7, 13), (64, 33)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        write_png(str(tmp_path / "a.png"), img)
        assert np.array_equal(read_png(str(tmp_path / "a.png")), img)
    write_png(str(tmp_path / "b.png"), img[:, ::2])                      # a strided view
    assert np.array_equal(read_png(str(tmp_path / "b.png")), img[:, ::2])


def test_prediction_files(tmp_path):
    inf = _inferencer()
    pred = {"labels": [3, 5], "scores": [0.9, 0.5], "bboxes": [[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.5, 8.0]]}
    inf.num_predicted_imgs = 7
    inf.save_outputs(pred, None, "", False)                               # no out_dir: nothing is written
    inf.save_outputs(pred, None, str(tmp_path), True)                     # no_save_pred
    assert os.listdir(tmp_path) == []
    inf.save_outputs(pred, np.zeros((2, 3, 3), np.uint8), str(tmp_path), False)
    assert sorted(os.listdir(tmp_path)) == ["preds", "vis"] and os.listdir(tmp_path / "preds") == ["7.json"]
    assert json.load(open(tmp_path / "preds" / "7.json")) == pred
    assert os.listdir(tmp_path / "vis") == ["00000000.png"] and read_png(str(tmp_path / "vis" / "00000000.png")).shape == (2, 3, 3)
