"""GPU: the appearance cue -- `codetr_appearance_describe_*` (csrc/appearance.hip), `codetr_track_update5_*`
(csrc/track.hip) and the Inferencer's `track_appearance="color"` -- against the numpy restatement
(tests/appearance_ref.py), bit for bit: every uint16 of the descriptors, the ids of every row, the whole decoded track state
and the appearance states, which sit between sentinel-filled guard rows."""
import functools

import numpy as np
import pytest
import torch

import appearance_cases as cases
import motion_sim_ref
import track_cases
from appearance_ref import TrackAppRef, TrackAssignAppRef, describe
from test_inferencer_batch_gpu import DEV, SWIN
from test_motion_gpu import _dets
from test_track_gpu import _assert_state

pytestmark = pytest.mark.gpu
REFS = dict(greedy=TrackAppRef, optimal=TrackAssignAppRef)
SENTINEL = 0x5A5A
T8 = dict(max_tracks=8)
PALETTE = dict(cases.COLOURS, yellow=(200, 200, 40), cyan=(40, 200, 200), magenta=(200, 40, 200), white=(230, 230, 230))


def _upload(frames):
    """the images in one flat buffer at non-zero offsets (7 bytes in front, 5 between) -> (buffer on the device, rows)"""
    parts, rows, at = [np.full(7, 0xA5, np.uint8)], [], 7
    for im in frames:
        rows.append((at, im.shape[0], im.shape[1]))
        parts += [np.ascontiguousarray(im).reshape(-1), np.full(5, 0xA5, np.uint8)]
        at += im.size + 5
    return torch.from_numpy(np.concatenate(parts)).to(DEV), rows


def _pack(dets, dtype, scores=None, labels=None, Q=None):
    """per frame a list of boxes (and of scores, labels; 0.9 and 0 by default) -> (Detections, labels, count)"""
    N = len(dets)
    Q = Q or max(1, max(len(b) for b in dets))
    boxes, sc = np.zeros((N, Q, 4), np.float32), np.zeros((N, Q), np.float32)
    lab, count = np.zeros((N, Q), np.int64), np.zeros(N, np.int32)
    for f, b in enumerate(dets):
        count[f] = len(b)
        boxes[f, :len(b)] = np.array(b, np.float32).reshape(-1, 4)
        sc[f, :len(b)] = 0.9 if scores is None else scores[f]
        lab[f, :len(b)] = 0 if labels is None else labels[f]
    return _dets(boxes, sc, lab, count, dtype), lab, count


def _scene(objects, seed=0, noise=6):
    """one 120 x 160 frame of the sequences' kind: objects = [(colour name, x, y)] -> (image, boxes)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(100, 140, (cases.H, cases.W, 3), dtype=np.int64)
    boxes = []
    for colour, x, y in objects:
        n = rng.integers(-noise, noise + 1, (cases.BH, cases.BW, 3), dtype=np.int64) if noise else 0
        img[y:y + cases.BH, x:x + cases.BW] = np.array(PALETTE[colour], np.int64) + n
        boxes.append((float(x), float(y), float(x + cases.BW), float(y + cases.BH)))
    return img.astype(np.uint8), boxes


def _slice(dets, a, b):
    from codetr import hip_ops

    return hip_ops.Detections(*(t[a:b] for t in dets[:4]), None)


def _run(frames, dets, labels, count, association="greedy", streams=None, S=1, settings=T8, app=None, motions=None,
         chunks=None, use=None, check_desc=True):
    """the frames through appearance_descriptors + track_update in launches of `chunks` rows (use: per chunk, whether the
    cue is given) and through the restatement; asserts ids, track states and appearance states equal -> (ids, refs, g)"""
    from codetr import hip_ops

    N, T = len(frames), settings["max_tracks"]
    streams = streams or [0] * N
    chunks = chunks or [N]
    use = use or [True] * len(chunks)
    state = hip_ops.new_track_state(S, T, DEV)
    guarded = hip_ops.new_appearance_state(S + 2, T, DEV)
    guarded[0].fill_(SENTINEL)
    guarded[-1].fill_(SENTINEL)
    astate = guarded[1:-1]
    m = None if motions is None else torch.tensor(np.asarray(motions, np.float32), device=DEV)
    ids, descs, used, at = [], [], [], 0
    for n, u in zip(chunks, use):
        buf, rows = _upload(frames[at:at + n])
        part = _slice(dets, at, at + n)
        d = hip_ops.appearance_descriptors(buf, rows, part)
        kw = dict(appearance=d, appearance_state=astate, appearance_settings=app) if u else {}
        ids.append(hip_ops.track_update(part, state, streams[at:at + n], settings, association,
                                        motion=None if m is None else m[at:at + n], **kw).cpu().numpy())
        descs.append(d.cpu().numpy().view(np.uint16))
        used += [u] * n
        at += n
    assert at == N
    ids, descs = np.concatenate(ids), np.concatenate(descs)
    refs = [REFS[association](settings, app) for _ in range(S)]
    want = np.zeros_like(ids)
    for f in range(N):
        if check_desc:
            assert np.array_equal(descs[f], describe(frames[f], dets.boxes[f].cpu(), count[f])), f
        want[f] = refs[streams[f]].update(dets.boxes[f].cpu(), dets.scores[f].cpu(), labels[f], count[f],
                                          motion=None if motions is None else motions[f], desc=descs[f] if used[f] else None)
    if ids.size <= 100:
        print("ids", ids.tolist())
    assert np.array_equal(ids, want), "ids"
    host = hip_ops.track_state_to_host(state)
    raw = guarded.cpu().numpy().view(np.uint16)
    assert (raw[0] == SENTINEL).all() and (raw[-1] == SENTINEL).all()      # the guard rows
    g = hip_ops.appearance_state_to_host(astate)
    assert g.dtype == np.uint16 and g.shape == (S, T, 128)
    for s, ref in enumerate(refs):
        _assert_state(host, s, ref.state())
        assert np.array_equal(g[s], ref.g), "appearance state"
    return ids, refs, g


@functools.lru_cache(maxsize=None)
def _sequence(name):
    frames, dets, names = cases.sequence(name)
    return list(frames), dets, names


# ---- 1. the descriptors -------------------------------------------------------------------------------------------------
def _geometry(Q, dtype, extra=()):
    images = [cases.edge_image(48, 64, 1), cases.edge_image(37, 53, 2)]
    frames = [images[n % 2] for n in range(4)]
    boxes = []
    for n, im in enumerate(frames):
        pool = cases.geometry_boxes(*im.shape[:2]) + list(extra)
        boxes.append([pool[(q + 3 * n) % len(pool)] if Q < len(pool) else pool[q % len(pool)] for q in range(Q)])
    dets, _, _ = _pack(boxes, dtype, Q=Q)
    count = torch.tensor([max(Q - 1, 0), 0, Q + 3, -2], dtype=torch.int32, device=DEV)
    return frames, dets._replace(count=count), count.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("Q", [1, 5, 67])
def test_descriptors(Q, dtype):
    """two images at non-zero offsets, boxes inside, over every edge, outside, larger, degenerate and non-finite; a count
    below Q, 0, above Q and negative; pixel values on both sides of every bin edge"""
    from codetr import _cabi, hip_ops

    extra = [(1e30, 2.0, 3e38, 9.0), (-1e30, -1e30, 1e30, 1e30), (5.0, 1e30, 9.0, 2e30)] if dtype == torch.float32 else []
    frames, dets, count = _geometry(Q, dtype, extra)
    buf, rows = _upload(frames)
    before = _cabi.CALLS["appearance_describe"]
    got = hip_ops.appearance_descriptors(buf, rows, dets)
    assert _cabi.CALLS["appearance_describe"] == before + 1
    assert got.dtype == torch.int16 and tuple(got.shape) == (4, Q, 128)
    got = got.cpu().numpy().view(np.uint16)
    some = 0
    for n in range(4):
        want = describe(frames[n], dets.boxes[n].cpu(), count[n])
        assert np.array_equal(got[n], want), n
        some += int(want.any(axis=1).sum())
    assert not got[1].any() and not got[3].any()
    assert some >= (1 if Q == 1 else 5)


def test_descriptors_33_rows_are_split():
    from codetr import _cabi, hip_ops

    images = [cases.edge_image(48, 64, 3), cases.edge_image(37, 53, 4)]
    frames = [images[n % 2] for n in range(33)]
    pool = cases.geometry_boxes(37, 53)
    dets, _, count = _pack([[pool[(n + q) % 11] for q in range(5)] for n in range(33)], torch.float32)
    buf, rows = _upload(images)
    before = _cabi.CALLS["appearance_describe"]
    got = hip_ops.appearance_descriptors(buf, [rows[n % 2] for n in range(33)], dets).cpu().numpy().view(np.uint16)
    assert _cabi.CALLS["appearance_describe"] == before + 2
    for n in range(33):
        assert np.array_equal(got[n], describe(frames[n], dets.boxes[n].cpu(), count[n])), n


# ---- 2. the tracker -----------------------------------------------------------------------------------------------------
def _expect(name, ids, names):
    full = list(range(1, len(cases.OBJECTS[name]) + 1))
    for f, present in enumerate(names):
        assert ids[f, :len(present)].tolist() == (full if len(present) == len(full) else [1]), f


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("association", ["greedy", "optimal"])
@pytest.mark.parametrize("name", ["reentry", "lanes"])
def test_sequences(name, association, dtype):
    from codetr import _cabi, hip_ops

    frames, boxes, names = _sequence(name)
    dets, labels, count = _pack(boxes, dtype)
    before = dict(_cabi.CALLS)
    ids, refs, g = _run(frames, dets, labels, count, association)
    assert _cabi.CALLS["track_update5"] == before["track_update5"] + 1
    assert _cabi.CALLS["track_update4"] == before["track_update4"] and _cabi.CALLS["track_update"] == before["track_update"]
    _expect(name, ids, names)
    assert refs[0].log["gated"] >= 1 and g[0, :len(cases.OBJECTS[name])].any(axis=1).all() and not g[0, 3:].any()
    # the plain tracker does lose the id
    plain = hip_ops.track_update(dets, hip_ops.new_track_state(1, 8, DEV), settings=T8, association=association).cpu().numpy()
    assert plain[-1, :len(names[-1])].tolist() == ([1, 3] if name == "reentry" else [1, 3, 2])


def test_sequence_bf16():
    frames, boxes, names = _sequence("lanes")
    dets, labels, count = _pack(boxes, torch.bfloat16)
    ids, _, _ = _run(frames, dets, labels, count, "greedy")
    _expect("lanes", ids, names)


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_chunking_does_not_matter(association):
    frames, boxes, names = _sequence("reentry")
    dets, labels, count = _pack(boxes, torch.float16)
    one, _, g1 = _run(frames, dets, labels, count, association)
    parts, _, g2 = _run(frames, dets, labels, count, association, chunks=[1, 3, 4, 16])
    assert np.array_equal(one, parts) and np.array_equal(g1, g2)


def test_two_streams_in_one_launch():
    """the rows of two cameras interleaved (48 rows: two launches), each with its own tracks and appearances"""
    fa, ba, na = _sequence("lanes")
    fb, bb, nb = _sequence("reentry")
    frames = [x for pair in zip(fa, fb) for x in pair]
    boxes = [x for pair in zip(ba, bb) for x in pair]
    dets, labels, count = _pack(boxes, torch.float32)
    ids, _, g = _run(frames, dets, labels, count, "greedy", streams=[0, 1] * 24, S=2)
    _expect("lanes", ids[0::2], na)
    _expect("reentry", ids[1::2], nb)
    assert not np.array_equal(g[0], g[1])


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_refusals_low_matches_and_frees(association):
    """max_tracks = 4 with six objects: two refusals per frame; then the objects leave one by one (slots are freed and
    zeroed), one comes back with a low score (match C: its appearance stays) and a new one starts in a freed slot"""
    names = ["red", "green", "blue", "yellow", "cyan", "magenta"]
    at = {c: (8 + 25 * k, 10 + 6 * k) for k, c in enumerate(names)}
    plan = [names] * 4 + [names[:3]] * 2 + [["red", "white"]] * 3 + [["red"]] * 2
    frames, boxes, scores = [], [], []
    for f, present in enumerate(plan):
        img, b = _scene([(c, *(at[c] if c in at else (120, 70))) for c in present], seed=f)
        frames.append(img)
        boxes.append(b)
        scores.append([0.3 if (c == "red" and f in (5, 9)) else 0.9 for c in present])
    dets, labels, count = _pack(boxes, torch.float32, scores=scores)
    settings = dict(max_tracks=4, num_frames_retain=2)
    ids, refs, g = _run(frames, dets, labels, count, association, settings=settings)
    log = refs[0].log
    assert log["refused"] >= 8 and log["C"] >= 2 and log["retired"] >= 2 and log["started"] >= 5
    # the low-score match of frame 5 left g as frame 4 had it
    _, refs4, g4 = _run(frames[:5], _slice(dets, 0, 5), labels[:5], count[:5], association, settings=settings)
    _, refs5, g5 = _run(frames[:6], _slice(dets, 0, 6), labels[:6], count[:6], association, settings=settings)
    assert refs5[0].log["C"] == 1 and np.array_equal(g4[0, 0], g5[0, 0]) and g4[0, 0].any()


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_two_candidates_of_identical_colour(association):
    """a lost track and two noiseless candidates of its colour at equal distances left and right of it: equal values"""
    frames, boxes = [], []
    for f in range(8):
        objs = [("red", 60, 40)] if f < 4 else ([] if f < 6 else [("red", 40, 40), ("red", 80, 40)])
        img, b = _scene(objs, seed=f, noise=0)
        frames.append(img)
        boxes.append(b)
    dets, labels, count = _pack(boxes, torch.float32, Q=2)
    ids, refs, _ = _run(frames, dets, labels, count, association)
    assert ids[6].tolist() == [1, -2] and ids[7].tolist() == [1, -2]      # the lower row wins the tie, the other starts
    if association == "greedy":
        assert refs[0].log["tie"] >= 1
    assert refs[0].log["gated"] >= 1


@pytest.mark.parametrize("app,issued", [(dict(appearance_thr=0.0), 2), (dict(appearance_thr=1.0), None),
                                        (dict(proximity_thr=0.0), 2), (dict(proximity_thr=1.0), 2), (dict(reid_gate=0.0), 3),
                                        (dict(reid_gate=0.25), 3)],
                         ids=["thr0", "thr1", "prox0", "prox1", "gate0", "gate_small"])
def test_settings(app, issued):
    frames, boxes, names = _sequence("reentry")
    dets, labels, count = _pack(boxes, torch.float16)
    for association in ("greedy", "optimal"):
        _, refs, _ = _run(frames, dets, labels, count, association, app=app)
        if issued is not None:
            assert refs[0].issued == issued


def test_label_mismatch_inside_the_gate():
    frames, boxes, names = _sequence("reentry")
    labels = [[0, 0] if f < 14 else [0, 1] for f in range(len(boxes))]
    dets, lab, count = _pack(boxes, torch.float32, labels=[l[:len(b)] for l, b in zip(labels, boxes)])
    ids, refs, _ = _run(frames, dets, lab, count, "greedy")
    assert refs[0].issued == 3 and ids[14].tolist() == [1, -3]


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_motion_rows_with_appearance(association):
    frames, boxes, names = _sequence("lanes")
    dets, labels, count = _pack(boxes, torch.float32)
    rows = [[0, 0, 0, 0, 0, 0, 0, 0], [1.5, -1.0, 1, 1, 1, 0, 0, 0], [0.5, 0.25, 1, 2, 1.0078125, 0.00390625, 80, 60],
            [float("nan"), 1, 1, 1, 1, 0, 0, 0]]
    motions = [rows[f % 4] for f in range(len(frames))]
    _run(frames, dets, labels, count, association, motions=motions, chunks=[8, 16])


def test_translation_motion_is_widened():
    """a [N, 4] motion with the cue == the same rows as [N, 8] with model = valid"""
    from codetr import hip_ops

    frames, boxes, names = _sequence("lanes")
    dets, labels, count = _pack(boxes, torch.float32)
    buf, rows = _upload(frames)
    desc = hip_ops.appearance_descriptors(buf, rows, dets)
    four = torch.tensor([[1.5 * (-1) ** f, 0.5, f % 3 != 0, 0] for f in range(len(frames))], dtype=torch.float32, device=DEV)
    eight = torch.cat([four[:, :3], four[:, 2:3], torch.full_like(four, 7.0)], 1)       # (a, b, px, py are not read)
    out = []
    for m in (four, eight):
        st, ast = hip_ops.new_track_state(1, 8, DEV), hip_ops.new_appearance_state(1, 8, DEV)
        out.append((hip_ops.track_update(dets, st, settings=T8, motion=m, appearance=desc, appearance_state=ast), st, ast))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    st = hip_ops.new_track_state(1, 8, DEV)
    hip_ops.track_update(dets, st, settings=T8, appearance=desc, appearance_state=hip_ops.new_appearance_state(1, 8, DEV))
    assert not torch.equal(st, out[0][1])                                                  # (the motion does move the state)


@pytest.mark.parametrize("association", ["greedy", "optimal"])
def test_without_descriptors_it_is_the_tracker_as_it_is(association):
    """codetr_track_update5_* with a NULL desc_dev: update4's ids and state bytes; hip_ops with appearance=None calls what
    it always called"""
    from codetr import _appearance, _assign, _cabi, hip_ops

    frames, boxes, names = _sequence("lanes")
    dets, labels, count = _pack(boxes, torch.float16)
    N = len(frames)
    four = torch.tensor([[1.5 * (-1) ** f, 0.5, f % 3 != 0, 0] for f in range(N)], dtype=torch.float32, device=DEV)
    eight = torch.tensor([[0.5, 0.25, 1, f % 3, 1.0078125, 0.00390625, 80, 60] for f in range(N)], dtype=torch.float32,
                         device=DEV)
    cfg = hip_ops.track_settings(T8)
    thr = (cfg["obj_score_thrs"]["high"], cfg["obj_score_thrs"]["low"], cfg["init_track_thr"], cfg["match_iou_thrs"]["high"],
           cfg["match_iou_thrs"]["low"], cfg["match_iou_thrs"]["tentative"])
    for motion in (None, four, eight):
        st = hip_ops.new_track_state(1, 8, DEV)
        before = dict(_cabi.CALLS)
        want = hip_ops.track_update(dets, st, settings=T8, association=association, motion=motion)
        assert _cabi.CALLS["track_update5"] == before["track_update5"]
        assert _cabi.CALLS["appearance_describe"] == before["appearance_describe"]
        wide = motion
        if motion is not None and motion.shape[1] == 4:
            wide = torch.cat([motion[:, :3], motion[:, 2:3], torch.zeros_like(motion)], 1).contiguous()
        st5 = hip_ops.new_track_state(1, 8, DEV)
        ids = torch.full((N, 3), 77, dtype=torch.int32, device=DEV)
        with torch.cuda.device(DEV):
            _appearance.track_update5(dets.boxes, dets.scores, dets.labels, dets.count, [0] * N, st5, 8, thr,
                                      cfg["num_frames_retain"], cfg["num_tentatives"], cfg["weight_iou_with_det_scores"], ids,
                                      _assign.ASSOCIATIONS[association], wide, None, None, None, None)
        assert torch.equal(ids, want) and torch.equal(st5, st)


def test_a_stream_switches_to_the_cue():
    """four frames without descriptors, then with: the live tracks' appearances are all zero, s = 0, and each adopts the
    descriptor of its first high match"""
    frames, boxes, names = _sequence("lanes")
    dets, labels, count = _pack(boxes, torch.float32)
    ids, refs, g = _run(frames, dets, labels, count, "greedy", chunks=[4, 20], use=[False, True])
    assert refs[0].log["adopted"] == 3 and g[0, :3].any(axis=1).all()
    _, refs4, g4 = _run(frames[:4], _slice(dets, 0, 4), labels[:4], count[:4], "greedy", use=[False])
    assert not g4.any()


def test_track_update_large_lds():
    """max_tracks = 512, Q = 1024: the kernel needs the opt-in to large LDS; the descriptors are the device's (compared
    above), of a noise image under the dense boxes"""
    b, s, l, c = track_cases.cached_sequence("dense")
    span = int(np.ceil(np.nanmax(np.where(np.isfinite(b), b, 0)))) + 2
    img = cases.edge_image(min(span, 700), min(span, 900), 9)
    dets = _dets(b, s, l, c, torch.float32)
    _, refs, g = _run([img] * len(c), dets, l, c, "greedy", settings=dict(max_tracks=512), check_desc=False,
                      app=dict(appearance_thr=0.25, proximity_thr=0.0))     # (every pair of one label is gated)
    assert refs[0].log["A"] > 256 and refs[0].log["refused"] > 0 and refs[0].log["added"] > 0


# ---- 3. arguments -------------------------------------------------------------------------------------------------------
def test_arguments():
    from codetr import _appearance, _assign, hip_ops

    frames, boxes, names = _sequence("lanes")
    frames, boxes = frames[:2], boxes[:2]
    dets, labels, count = _pack(boxes, torch.float32)
    buf, rows = _upload(frames)
    desc = hip_ops.appearance_descriptors(buf, rows, dets)
    st, ast = hip_ops.new_track_state(1, 8, DEV), hip_ops.new_appearance_state(1, 8, DEV)
    ok = dict(appearance=desc, appearance_state=ast)
    for bad in (dict(appearance=desc), dict(appearance_state=ast), dict(ok, appearance=desc.float()),
                dict(ok, appearance=desc[:, :2]), dict(ok, appearance=desc.cpu()), dict(ok, appearance=desc.cpu().numpy()),
                dict(ok, appearance_state=hip_ops.new_appearance_state(1, 4, DEV)),
                dict(ok, appearance_state=hip_ops.new_appearance_state(2, 8, DEV)),
                dict(ok, appearance_state=ast.view(torch.uint8)), dict(ok, appearance_state=ast.cpu()),
                dict(ok, appearance_settings=dict(reid_gate=-1)), dict(ok, appearance_settings=dict(gate=1))):
        with pytest.raises(ValueError):
            hip_ops.track_update(dets, st, settings=T8, **bad)
    with pytest.raises(ValueError):
        hip_ops.appearance_descriptors(buf, [(rows[0][0], 120, 160), (rows[1][0] + 6, 120, 160)], dets)   # past the buffer
    with pytest.raises(ValueError):
        hip_ops.appearance_descriptors(buf, rows[:1], dets)
    with pytest.raises(ValueError):
        hip_ops.appearance_descriptors(buf, rows, dets._replace(boxes=dets.boxes.double()))
    for bad in ((0, 8), (1, 0), (1, 513)):
        with pytest.raises(ValueError):
            hip_ops.new_appearance_state(*bad, DEV)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not ast.cpu().numpy().any()                       # nothing was launched

    # the entry points' own checks
    assert _appearance.state_bytes(8) == 2048 and _appearance.state_bytes(0) < 0 and _appearance.state_bytes(513) < 0
    assert _appearance.work_bytes(2, 8, 3) == 4 * 2 * 8 * 3 and _appearance.work_bytes(1, 8, 1025) < 0
    assert _appearance.work_bytes(0, 8, 3) < 0 and _appearance.work_bytes(1, 513, 3) < 0
    out = torch.full((2, 3, 128), 7, dtype=torch.int16, device=DEV)
    with torch.cuda.device(DEV):
        with pytest.raises(RuntimeError, match=r"code -1\)"):
            _appearance.describe(buf, [rows[0], (rows[1][0] + 6, 120, 160)], dets.boxes, dets.count, out)   # past src_bytes
        with pytest.raises(RuntimeError, match=r"code -1\)"):
            _appearance.describe(buf, [rows[0], (rows[1][0], 0, 160)], dets.boxes, dets.count, out)
        with pytest.raises(RuntimeError, match=r"code -3\)"):
            _appearance.describe(buf, [rows[0], (0, 1, 32768)], dets.boxes, dets.count, out)
        big = torch.zeros((33, 1, 4), device=DEV)
        with pytest.raises(RuntimeError, match=r"code -3\)"):
            _appearance.describe(buf, [rows[0]] * 33, big, torch.zeros(33, dtype=torch.int32, device=DEV),
                                 torch.zeros((33, 1, 128), dtype=torch.int16, device=DEV))
        cfg = hip_ops.track_settings(T8)
        thr = (0.6, 0.1, 0.7, 0.1, 0.5, 0.3)
        ids = torch.full((2, 3), 7, dtype=torch.int32, device=DEV)
        work = torch.empty(_appearance.work_bytes(1, 8, 3), dtype=torch.uint8, device=DEV)
        head = (dets.boxes, dets.scores, dets.labels, dets.count, [0, 0], st, 8, thr, cfg["num_frames_retain"],
                cfg["num_tentatives"], True, ids, _assign.ASSOCIATIONS["greedy"], None)
        for tail in ((desc, None, (0.75, 0.5, 1.5), work), (desc, ast, None, work), (desc, ast, (0.75, 0.5, 1.5), None),
                     (desc, ast, (0.75, 0.5, 1.5), work[:-1]), (desc, ast, (1.5, 0.5, 1.5), work),
                     (desc, ast, (0.75, -0.1, 1.5), work), (desc, ast, (0.75, 0.5, -1.0), work),
                     (desc, ast, (0.75, 0.5, float("nan")), work), (desc.view(-1)[2:2 + 2 * 3 * 128], ast, (0.75, 0.5, 1.5), work)):
            with pytest.raises(RuntimeError, match=r"code -1\)"):
                _appearance.track_update5(*head, *tail)
    torch.cuda.synchronize()
    assert (out == 7).all() and (ids == 7).all() and not st.cpu().numpy().any() and not ast.cpu().numpy().any()


# ---- 4. the Inferencer --------------------------------------------------------------------------------------------------
def _patched(frames):
    """the frames with their number k in a constant 8 x 8 corner patch (red = 8 k)"""
    out = []
    for k, f in enumerate(frames):
        f = f.copy()
        f[:8, :8] = (8 * k, 100, 50)
        out.append(f)
    return out


def _stub(inf, name):
    """a scripted model: reads the frame number from the corner patch and returns the sequence's boxes of that frame (in
    the coordinates of the resized image) with scores 0.95, 0.94, .. in object order; a hidden object is a row of score 0.02"""
    from codetr.inferencer import rescale_size

    mean, std = inf.mean[0], inf.std[0]
    nh, nw = rescale_size(cases.H, cases.W, inf.scale)
    objects = cases.OBJECTS[name]
    F = cases.FRAMES[name]
    table, scores = torch.zeros((F, len(objects), 4)), torch.full((F, len(objects)), 0.02)
    for f in range(F):
        for k, obj in enumerate(objects):
            p = cases.position(name, obj, f)
            table[f, k] = torch.tensor([150.0, 110.0, 158.0, 118.0] if p is None else
                                       [p[0], p[1], p[0] + cases.BW, p[1] + cases.BH])
            if p is not None:
                scores[f, k] = 0.95 - 0.01 * k

    def model(x, m):
        N = x.shape[0]
        k = torch.round((x[:, 0, 0, 0].float() * std + mean) / 8).long().clamp(0, F - 1).cpu()
        boxes = table[k] * torch.tensor([nw / cases.W, nh / cases.H] * 2)
        return boxes.to(x.device, x.dtype), scores[k].to(x.device, x.dtype).contiguous(), torch.zeros(
            (N, len(objects)), dtype=torch.long, device=x.device)
    return model


def _inferencer(name, **kw):
    from codetr.inferencer import Inferencer

    inf = Inferencer(None, SWIN, dataset_meta=None, **kw)
    inf.model = _stub(inf, name)
    return inf


def _reference_run(frames, preds, motion=False):
    est, ref, ids = motion_sim_ref.MotionSimRef(), TrackAppRef(), []
    for img, p in zip(frames, preds):
        n = len(p["labels"])
        boxes = np.asarray(p["bboxes"], np.float32).reshape(n, 4)
        ids.append(ref.update(boxes, np.asarray(p["scores"], np.float32), np.asarray(p["labels"], np.int64),
                              motion=est.estimate(img)[0] if motion else None, desc=describe(img, boxes)).tolist())
    return ids


def _kept(name, preds, names):
    full = list(range(1, len(cases.OBJECTS[name]) + 1))
    return all(p["track_ids"][:len(n)] == (full if len(n) == len(full) else [1]) for p, n in zip(preds, names))


@pytest.mark.parametrize("name", ["reentry", "lanes"])
def test_inferencer_keeps_the_ids(name):
    from codetr import _cabi

    raw, _, names = _sequence(name)
    frames = _patched(raw)
    inf = _inferencer(name, tracker={}, track_appearance="color")
    before = dict(_cabi.CALLS)
    preds = inf(frames[:10], device=DEV, dtype=torch.float32, batch_size=8)["predictions"]       # chunks of 8 + 2, then 8 + 6
    preds += inf(frames[10:], device=DEV, dtype=torch.float32, batch_size=8)["predictions"]
    assert _cabi.CALLS["appearance_describe"] == before["appearance_describe"] + 4
    assert _cabi.CALLS["track_update5"] == before["track_update5"] + 4
    assert _cabi.CALLS["track_update"] == before["track_update"] and _cabi.CALLS["track_update4"] == before["track_update4"]
    assert [p["track_ids"] for p in preds] == _reference_run(frames, preds)
    assert _kept(name, preds, names)
    assert all(set(p) == {"labels", "scores", "bboxes", "track_ids"} for p in preds)              # no new key
    plain = _inferencer(name, tracker={})(frames, device=DEV, dtype=torch.float32, batch_size=8)["predictions"]
    assert not _kept(name, plain, names)
    optimal = _inferencer(name, tracker={}, track_association="optimal", track_appearance=dict(type="color", reid_gate=2.0))
    assert _kept(name, optimal(frames, device=DEV, dtype=torch.float32, batch_size=5)["predictions"], names)


def test_inferencer_two_cameras_and_reset():
    raw, _, names = _sequence("reentry")
    frames = _patched(raw)
    order = [k for pair in zip(range(0, 22), range(2, 24)) for k in pair]      # camera 5: frames 0..21, camera 2: frames 2..23
    inf = _inferencer("reentry", tracker={}, track_appearance="color")
    preds = inf([frames[k] for k in order], device=DEV, dtype=torch.float32, batch_size=6, streams=[5, 2] * 22)["predictions"]
    for cam in (0, 1):
        mine = [frames[k] for k in order[cam::2]]
        assert [p["track_ids"] for p in preds[cam::2]] == _reference_run(mine, preds[cam::2])
    assert _kept("reentry", preds[0::2], names[:22])
    state = inf._appearance_state.cpu().numpy()
    rows = inf._track_rows
    assert state[rows[5]].any() and state[rows[2]].any() and inf._appearance_state.shape[0] == inf._track_state.shape[0]
    inf.reset_tracks(5)
    state = inf._appearance_state.cpu().numpy()
    assert not state[rows[5]].any() and state[rows[2]].any()
    again = inf(frames[14:16], device=DEV, dtype=torch.float32, batch_size=2, streams=5)["predictions"]
    assert [p["track_ids"] for p in again] == [[1, 2], [1, 2]]                     # a fresh stream: frame 0 confirms at once
    inf.reset_tracks()
    assert inf._appearance_state is None and inf._track_state is None


def test_inferencer_describes_before_it_draws():
    """with a visualizer the boxes are drawn into the buffer the descriptors are gathered from: the gather comes first"""
    raw, _, names = _sequence("lanes")
    frames = _patched(raw)
    kw = dict(tracker={}, track_appearance="color")
    plain = _inferencer("lanes", **kw)(frames, device=DEV, dtype=torch.float32, batch_size=8)["predictions"]
    inf = _inferencer("lanes", visualizer=dict(classes=["thing"], line_width=5), **kw)
    out = inf(frames, return_vis=True, pred_score_thr=0.3, device=DEV, dtype=torch.float32, batch_size=8)
    assert any(not np.array_equal(v, f) for v, f in zip(out["visualization"], frames))        # something was drawn
    assert [p["track_ids"] for p in out["predictions"]] == [p["track_ids"] for p in plain]
    assert _kept("lanes", plain, names)


def test_inferencer_with_camera_motion():
    from codetr import _cabi

    raw, _, names = _sequence("lanes")
    frames = _patched(raw)
    inf = _inferencer("lanes", tracker={}, track_appearance="color", track_motion="similarity")
    before = dict(_cabi.CALLS)
    preds = inf(frames, device=DEV, dtype=torch.float32, batch_size=8)["predictions"]
    assert _cabi.CALLS["track_update5"] == before["track_update5"] + 3 and _cabi.CALLS["motion_estimate2"] == before["motion_estimate2"] + 3
    assert [p["track_ids"] for p in preds] == _reference_run(frames, preds, motion=True)
    assert all("camera_motion" in p for p in preds)
    inf = _inferencer("lanes", tracker={}, track_appearance="color", track_motion="translation")
    preds = inf(frames, device=DEV, dtype=torch.float32, batch_size=8)["predictions"]
    assert len(preds) == len(frames) and all("camera_transform" not in p for p in preds)


def test_inferencer_without_the_cue_calls_what_it_called():
    from codetr import _cabi
    from codetr.inferencer import Inferencer

    raw, _, names = _sequence("lanes")
    frames = _patched(raw)[:8]
    inf = _inferencer("lanes", tracker={})
    assert inf.track_appearance is None
    before = dict(_cabi.CALLS)
    inf(frames, device=DEV, dtype=torch.float32, batch_size=4)
    delta = {k: v - before[k] for k, v in _cabi.CALLS.items() if v != before[k]}
    assert delta["track_update"] == 2 and "track_update5" not in delta and "appearance_describe" not in delta
    assert inf._appearance_state is None
    with pytest.raises(ValueError):
        Inferencer(None, SWIN, dataset_meta=None, track_appearance="color")                      # no tracker
    for bad in ("reid", dict(type="color", reid_gate=-1), dict(type="colour")):
        with pytest.raises(ValueError):
            Inferencer(None, SWIN, dataset_meta=None, tracker={}, track_appearance=bad)
