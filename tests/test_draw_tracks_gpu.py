"""GPU: `codetr_trail_update_*`, `codetr_draw_tracks_*` and the Inferencer's `tracks` setting against
tests/draw_tracks_ref.py, byte for byte: the state after each launch, every snapshot, every image and guard byte."""
import numpy as np
import pytest
import torch

import draw_ref as D
import draw_tracks_ref as R
from test_inferencer_batch_gpu import DEV
from test_track_gpu import _frames, _inferencer, _reference_ids

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
CLASSES, PALETTE = ["person", "car", "dog"], [(255, 0, 0), (0, 255, 0), (30, 60, 250)]
INF = float("inf")


def _dets(boxes, scores, labels, count):
    from codetr import hip_ops

    return hip_ops.Detections(boxes.to(DEV), scores.to(DEV), torch.as_tensor(labels).to(DEV),
                              torch.as_tensor(count, dtype=torch.int32).to(DEV), None)


# ---- 1. the trail rule: T = 2, K = 4, retain = 2; stream 0 has five frames (a..e), stream 1 two (p, q) ------------------------
# a: three ids, two entries (5 is dropped), the row beyond count is not read   b: 2 is gone; -4 finds no free entry
# c: 2 is freed (f - last = 2) and 3 -- its lower row is not finite -- reuses the entry   d: 1 twice, the lower row counts
# e: the fifth point of 1 wraps its ring   p, q: -7 is tentative; with it on, 7 in q is a duplicate of its key
IDS = dict(a=[1, 2, 5, 0, 0, 0, 0, 9], b=[1, -4, 0, 0, 0, 0, 0, 0], c=[3, 3, 1, 0, 0, 0, 0, 0], d=[1, 0, 1, 3, 0, 0, 0, 0],
           e=[0, 1, 0, 0, 0, 0, 0, 0], p=[-7, 9, 0, 0, 0, 0, 0, 0], q=[-7, 9, 7, 0, 0, 0, 0, 0])
COUNT = dict(a=7, b=100, c=8, d=8, e=2, p=2, q=3)
LAUNCHES = (("apb", [0, 1, 0]), ("cdqe", [0, 0, 1, 0]))


@pytest.mark.parametrize("tentative", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_trail_rule(dtype, tentative):
    from codetr import _cabi, hip_ops

    st = dict(trail=4, retain=2, tentative=tentative, anchor="bottom" if tentative else "center")
    rng = np.random.default_rng(3)
    boxes = {k: torch.tensor(np.round(rng.uniform(-40, 300, (8, 4)) * 4) / 4).to(dtype) for k in IDS}
    boxes["c"][0, 2] = INF
    state, refs = hip_ops.new_trail_state(2, 2, 4, DEV), [R.Trails(2, 4), R.Trails(2, 4)]
    for n, (frames, streams) in enumerate(LAUNCHES):
        dets = _dets(torch.stack([boxes[k] for k in frames]), torch.ones(len(frames), 8, dtype=dtype),
                     np.zeros((len(frames), 8), np.int64), [COUNT[k] for k in frames])
        ids = torch.tensor([IDS[k] for k in frames], dtype=torch.int32, device=DEV)
        before = _cabi.CALLS["trail_update"]
        got = hip_ops.trail_update(dets, ids, state, streams, st).cpu().numpy()
        assert _cabi.CALLS["trail_update"] == before + 1
        for row, (k, s) in enumerate(zip(frames, streams)):
            want = refs[s].update(boxes[k].float().numpy(), IDS[k], COUNT[k], 2, st["anchor"], tentative)
            assert np.array_equal(got[row], want), (n, k)
        assert np.array_equal(state.cpu().numpy(), np.stack([r.state() for r in refs])), n
    a = refs[0]
    assert a.f == 5 and a.id.tolist() == [1, 3] and a.len.tolist() == [4, 2] and a.head.tolist() == [1, 0]   # wrapped, reused
    assert refs[1].id.tolist() == ([7, 9] if tentative else [9, 7]) and refs[1].len.tolist() == [2, 2 if tentative else 1]


def test_trail_rule_at_the_limits():
    """T = 512, K = 64, Q = 1024: the state passes 64 KB of LDS; 600 new ids rank over several rounds of 256 threads and
    88 find no entry; the second row appends to entries in any order, with duplicates"""
    from codetr import hip_ops

    rng = np.random.default_rng(5)
    boxes = torch.tensor(np.round(rng.uniform(0, 2000, (2, 1024, 4)) * 2) / 2, dtype=torch.float32)
    ids = np.zeros((2, 1024), np.int32)
    ids[0, rng.permutation(1024)[:600]] = rng.permutation(np.arange(1, 601))
    ids[1] = rng.integers(300, 700, 1024)
    state, ref = hip_ops.new_trail_state(1, 512, 64, DEV), R.Trails(512, 64)
    dets = _dets(boxes, torch.ones(2, 1024), np.zeros((2, 1024), np.int64), [1024, 1000])
    got = hip_ops.trail_update(dets, torch.from_numpy(ids).to(DEV), state, 0, dict(trail=64)).cpu().numpy()
    for n in range(2):
        assert np.array_equal(got[n], ref.update(boxes[n].numpy(), ids[n], [1024, 1000][n])), n
    assert np.array_equal(state.cpu().numpy()[0], ref.state()) and ref.id.all() and (ref.len == 2).sum() > 100


# ---- 2. the drawing: tiles of 64 x 16, images of 130 x 37 and 65 x 16 at odd offsets between guard bytes ----------------------
ROWS = [(1, 37, 130), (1 + 37 * 130 * 3 + 4, 16, 65)]
TRAILS = [[(1, [(5, 5), (70, 5), (70, 34), (100, 4)]),                 # horizontal, vertical, a diagonal: every tile edge
           (2, [(10, 30), (40, 10), (40, 10), (41, 10), (41, 11)]),      # the other diagonal, zero length, a joint in a pixel
           (3, [(60, 12), (68, 20)]),                                    # through the tile corner (64, 16)
           (70, [(-10, 8), (20, -6), (140, 20), (110, 45)]),             # leaves on every side; colour (70 - 1) % 64
           (5, [(128, 36)])],                                            # one point: a disc
          [(1, [(0, 0), (64, 15)]), (2, [(64, 8)])]]
BOXES = [[10, 4, 60, 30], [50, 10, 120, 36], [-5, -5, 20, 12], [66, 2, 128, 15], [90, 20, 110, 30], [0, 0, 0, 0]]
DET_IDS = [3, -12, 0, 2147483647, 0, 7]
SCORES, LABELS = [0.9, 0.873, 0.5, 1.0, 0.1, 0.05], [0, 1, 2, 0, 1, 2]
TRACK_PALETTE = [(7 * i % 256, 255 - 3 * i, 40 + i) for i in range(64)]


def _snapshots(T, K):
    out = np.zeros((len(TRAILS), T, 4 + K), np.int32)
    for n, trails in enumerate(TRAILS):
        for t, (i, pts) in zip((1, 2, 4, 5, 7), trails):              # (free entries in between)
            p = np.zeros((K, 2), np.int16)
            p[:len(pts)] = pts
            box = np.array([*np.min(pts, 0), *np.max(pts, 0)], np.int16)
            out[n, t] = np.concatenate(([i, len(pts)], box.view(np.int32), p.reshape(-1).view(np.int32)))
    flat = [np.ascontiguousarray(out[:, :, a:b]).reshape(len(TRAILS), -1) for a, b in ((0, 1), (1, 2), (2, 4), (4, 4 + K))]
    return np.concatenate(flat, 1).view(np.uint8)


@pytest.mark.parametrize("style", [dict(trail_width=1), dict(trail_width=2, color_by="class", show_id=False, untracked=False),
                                   dict(trail_width=15, untracked=False, trail_alpha=1.0, line_width=1, font_scale=2)],
                         ids=["w1", "w2", "w15"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_drawing(dtype, style):
    from codetr import _cabi, hip_ops

    st = dict(style, trail=5)
    buf = np.random.default_rng(1).integers(0, 256, ROWS[1][0] + 16 * 65 * 3 + 5, dtype=np.uint8)
    boxes, scores = torch.tensor([BOXES, BOXES], dtype=torch.float32).to(dtype), torch.tensor([SCORES, SCORES]).to(dtype)
    labels, count, ids = np.array([LABELS, LABELS]), [6, 5], np.array([DET_IDS, DET_IDS[::-1]], np.int32)
    snaps = _snapshots(8, 5)
    assert [R.snapshot_trails(s, 8, 5)[0][0] for s in snaps] == [1, 1]
    dev = torch.from_numpy(buf).to(DEV)
    hip_ops.draw_tracks(dev, ROWS, _dets(boxes, scores, labels, count), torch.from_numpy(ids).to(DEV),
                        torch.from_numpy(snaps).to(DEV), hip_ops.draw_names_table(CLASSES).to(DEV),
                        torch.tensor(PALETTE, dtype=torch.uint8, device=DEV),
                        torch.tensor(TRACK_PALETTE, dtype=torch.uint8, device=DEV), st)
    want = R.draw_buffer(buf, ROWS, boxes.float().numpy(), scores.float().numpy(), labels, count, ids, TRAILS, CLASSES,
                         PALETTE, TRACK_PALETTE, _cabi.draw_font(), st)
    assert (want != buf).sum() > 3000 and np.array_equal(dev.cpu().numpy(), want)   # images and guard bytes


@pytest.mark.parametrize("dtype", DTYPES)
def test_untracked_rows_without_trails_are_draw_detections(dtype):
    from codetr import hip_ops

    buf = torch.from_numpy(np.random.default_rng(2).integers(0, 256, ROWS[1][0] + 16 * 65 * 3 + 5, dtype=np.uint8)).to(DEV)
    dets = _dets(torch.tensor([BOXES, BOXES], dtype=torch.float32).to(dtype), torch.tensor([SCORES, SCORES]).to(dtype),
                 np.array([LABELS, LABELS]), [6, 6])
    names, colors = hip_ops.draw_names_table(CLASSES).to(DEV), torch.tensor(PALETTE, dtype=torch.uint8, device=DEV)
    plain = hip_ops.draw_detections(buf.clone(), ROWS, dets, names, colors, dict(line_width=2))
    got = hip_ops.draw_tracks(buf.clone(), ROWS, dets, torch.zeros((2, 6), dtype=torch.int32, device=DEV), None, names, colors,
                              colors, dict(line_width=2, untracked=True))
    assert not torch.equal(plain, buf) and torch.equal(got, plain)


# ---- 3. the Inferencer: the stub model of the tracker's tests, six frames in two calls of three --------------------------------
def test_inferencer_tracks():
    from codetr import _cabi
    from codetr.inferencer import generated_palette

    frames, font = _frames(range(6)), _cabi.draw_font()
    inf = _inferencer(tracker={}, visualizer=dict(tracks=dict(trail=4, trail_width=3)))
    kw = dict(return_vis=True, device=DEV, dtype=torch.float16, batch_size=3)
    before = (_cabi.CALLS["trail_update"], _cabi.CALLS["draw_tracks"], _cabi.CALLS["draw_detections"])
    outs = [inf(frames[:3], **kw), inf(frames[3:], **kw)]
    assert (_cabi.CALLS["trail_update"], _cabi.CALLS["draw_tracks"], _cabi.CALLS["draw_detections"]) == \
        (before[0] + 2, before[1] + 2, before[2])
    names, palette, tp = inf.visualizer["classes"], inf.visualizer["palette"], generated_palette(64)

    def compose(preds, images):      # track ref, then trail ref, then draw ref
        want_ids, _ = _reference_ids(preds)
        trails, out = R.Trails(256, 4), []
        for p, ids, image in zip(preds, want_ids, images):
            assert p["track_ids"] == ids
            b = np.asarray(p["bboxes"], np.float32).reshape(-1, 4)
            snap = trails.update(b, ids, len(ids), 30)
            out.append(R.draw(image, b, p["scores"], p["labels"], ids, R.snapshot_trails(snap, 256, 4), names,
                              palette, tp, font, dict(trail=4, trail_width=3)))
        return out, trails

    preds, vis = outs[0]["predictions"] + outs[1]["predictions"], outs[0]["visualization"] + outs[1]["visualization"]
    want, trails = compose(preds, frames)
    assert trails.len.max() == 4 and trails.head.max() > 0                     # continued across the calls, and wrapped
    assert all(np.array_equal(g, w) for g, w in zip(vis, want)) and not np.array_equal(vis[5], frames[5])
    inf.reset_tracks()                                                         # the trails are gone with the tracks
    again = inf(frames[:1], **kw)
    assert np.array_equal(again["visualization"][0], compose(again["predictions"], frames[:1])[0][0])
    # without the key: the entry points of before, no new launch
    before = (_cabi.CALLS["trail_update"], _cabi.CALLS["draw_tracks"])
    plain = _inferencer(tracker={}, visualizer={})(frames[:3], **kw)
    assert (_cabi.CALLS["trail_update"], _cabi.CALLS["draw_tracks"]) == before
    for p, g, image in zip(plain["predictions"], plain["visualization"], frames):
        assert np.array_equal(g, D.draw(image, np.asarray(p["bboxes"], np.float32).reshape(-1, 4), p["scores"], p["labels"],
                                        names, palette, font))
