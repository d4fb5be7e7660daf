"""CPU: the restatement's integer capsule test (tests/draw_tracks_ref.py, include/codetr_draw_tracks.h) against exact
rational distance, and what of the host side runs without a GPU: the settings, the Inferencer's argument, the binding's
table against the header, the launchers' argument checks."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import draw_tracks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIN = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")
SEGMENTS = [((3, 4), (19, 4)), ((11, 2), (11, 21)), ((2, 3), (20, 18)), ((21, 5), (4, 17)), ((9, 9), (9, 9)),
            ((-7, 10), (30, 13)), ((5, 20), (6, 21))]


@pytest.mark.parametrize("p0,p1", SEGMENTS)
def test_capsule_is_exact_distance(p0, p1):
    """covered <=> the squared distance to the segment, as a fraction, is <= w^2 / 4"""
    d = (p1[0] - p0[0], p1[1] - p0[1])
    L = d[0] * d[0] + d[1] * d[1]
    for w in range(1, 16):
        mask = R.trail_mask(24, 24, [p0, p1], w)
        for y in range(24):
            for x in range(24):
                s = min(max(Fraction((x - p0[0]) * d[0] + (y - p0[1]) * d[1], L), 0), 1) if L else 0
                dist2 = (x - p0[0] - s * d[0]) ** 2 + (y - p0[1] - s * d[1]) ** 2
                assert bool(mask[y, x]) == (dist2 <= Fraction(w * w, 4)) == bool(R.covers(x, y, p0, p1, w)), (x, y, w)
    # the header's bound, at its corner: nothing passes 2^62
    cross = 16383 * 32767 + 16383 * 32767
    assert 2 * 32767 ** 2 < 2 ** 31 and cross < 2 ** 31 and cross ** 2 < 2 ** 62 and 225 * 2 ** 31 < 2 ** 39


def test_settings():
    from codetr import hip_ops

    assert hip_ops.TRAILS == R.DEFAULTS and hip_ops.trail_settings() == hip_ops.TRAILS
    assert hip_ops.trail_settings(dict(trail=0, trail_width=15, anchor="bottom"))["trail"] == 0
    assert hip_ops.TRAIL_ANCHORS == ("center", "bottom") and hip_ops.TRAIL_COLOR_BY == ("class", "track")
    bad = dict(color_by=["id", 1], anchor=["top", None], trail=[1, 65, -2, 2.5, "30", True], trail_width=[0, 16, 1.5],
               trail_alpha=[-0.1, 1.5, "a", float("nan")], retain=[0, 1.5, None], show_id=[1, "yes"], tentative=[0],
               untracked=[None])
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                hip_ops.trail_settings({key: v})
    with pytest.raises(ValueError, match="fade"):
        hip_ops.trail_settings(dict(fade=True))
    assert hip_ops.new_trail_state(3, 2, 4, "cpu").shape == (3, 16 + 16 * 2 + 4 * 2 * 4) and hip_ops.trail_snapshot_bytes(256, 30) == 34816
    for args in ((0, 2, 4), (1, 0, 4), (1, 513, 4), (1, 2, 1), (1, 2, 65)):
        with pytest.raises(ValueError):
            hip_ops.new_trail_state(*args, "cpu")


def test_inferencer_argument():
    from codetr.inferencer import Inferencer, generated_palette

    assert Inferencer(None, SWIN, None, visualizer={}, tracker={}).tracks is None
    inf = Inferencer(None, SWIN, None, visualizer=dict(tracks=True, line_width=2), tracker=dict(num_frames_retain=7))
    assert inf.tracks["style"] == dict(R.DEFAULTS, retain=7) and inf.tracks["palette"] == generated_palette(64)
    assert inf.visualizer["style"]["line_width"] == 2 and tuple(inf.tracks["colors"].shape) == (64, 3)
    inf = Inferencer(None, SWIN, None, tracker={}, visualizer=dict(tracks=dict(trail=0, retain=3, palette=[(1, 2, 3)])))
    assert inf.tracks["style"]["trail"] == 0 and inf.tracks["style"]["retain"] == 3 and inf.tracks["palette"] == [(1, 2, 3)]
    for tracks, key in ((dict(trail=1), "trail"), (dict(colour_by="track"), "colour_by"), (dict(palette=[]), "palette"),
                        (dict(palette=[(0, 0, 256)]), "palette"), ("on", "tracks")):
        with pytest.raises(ValueError, match=key):
            Inferencer(None, SWIN, None, tracker={}, visualizer=dict(tracks=tracks))
    with pytest.raises(ValueError, match="tracker"):
        Inferencer(None, SWIN, None, visualizer=dict(tracks=True))


def test_header_and_binding():
    from codetr import _cabi, _cheader, _draw_tracks, _redact

    text = open(os.path.join(ROOT, "include", "codetr_draw_tracks.h")).read()
    functions, defines = _cheader.parse(text)
    assert list(functions) == ["codetr_draw_tracks_abi_version", "codetr_trail_state_bytes", "codetr_trail_snapshot_bytes"] + \
        [f"codetr_{stem}_{t}" for stem in ("trail_update", "draw_tracks") for t in ("f16", "bf16", "f32")]
    assert defines == dict(CODETR_DRAW_TRACKS_ABI_VERSION=1, CODETR_TRAIL_MIN_LENGTH=2, CODETR_TRAIL_MAX_LENGTH=64,
                           CODETR_TRAIL_CENTER=0, CODETR_TRAIL_BOTTOM=1, CODETR_COLOR_BY_CLASS=0, CODETR_COLOR_BY_TRACK=1)
    assert set(_draw_tracks.SIGNATURES) == set(functions) and _draw_tracks.ABI_VERSION == 1
    i, l, p, u, f = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    assert _draw_tracks.SIGNATURES["codetr_trail_state_bytes"] == (l, [l, l])
    draw = _cabi.SIGNATURES["codetr_draw_detections_f16"]
    for t in ("f16", "bf16", "f32"):
        assert _draw_tracks.SIGNATURES["codetr_trail_update_" + t] == (i, [p, p, p, p, p, l, l, p, l, p, l, l, p, l, i, i, p])
        assert _draw_tracks.SIGNATURES["codetr_draw_tracks_" + t] == (i, draw[1] + [p, p, l, l, p, l, i, f, i, i, i])
    assert not set(functions) & (set(_cabi.SIGNATURES) | set(_redact.SIGNATURES))   # a companion: the others are untouched
    assert _cabi.ABI_VERSION == 54 and _redact.ABI_VERSION == 1
    text = " ".join(text.replace("\n *", " ").split())
    for phrase in ("cross^2 < 2^62", "EVERY COVERED PIXEL IS BLENDED ONCE PER TRAIL", "16 + 16 T + 4 T K", "not antialiased",
                   "only the one with the lowest j counts", "(w * w * L) / 4", "is unpinned", "does not move them"):
        assert phrase in text, phrase


def test_argument_checks_return_before_any_hip_call():
    """the launchers' checks are host code (csrc/draw_tracks_args.h): every rejected call returns its code without a GPU"""
    from codetr import _draw_tracks

    lib = _draw_tracks.load()
    assert lib.codetr_draw_tracks_abi_version() == 1 and lib.codetr_trail_state_bytes(512, 64) == 16 + 16 * 512 + 4 * 512 * 64
    assert lib.codetr_trail_snapshot_bytes(2, 4) == 64 and _draw_tracks.state_bytes(2, 4) == 80
    for T, K in ((0, 4), (513, 4), (2, 1), (2, 65)):
        assert lib.codetr_trail_state_bytes(T, K) == -1 and lib.codetr_trail_snapshot_bytes(T, K) == -1
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)
    streams = (ctypes.c_int * 2)(1, 0)
    good = dict(stream=None, boxes=one, scores=None, labels=None, count=one, N=2, Q=8, streams=streams, S=2, state=one, T=2,
                K=4, ids=one, retain=2, anchor=0, tentative=0, out=one)
    for kw, code in ((dict(boxes=None), -1), (dict(count=None), -1), (dict(streams=None), -1), (dict(state=None), -1),
                     (dict(ids=None), -1), (dict(out=None), -1), (dict(N=0), -1), (dict(Q=0), -1), (dict(S=1), -1),
                     (dict(T=0), -1), (dict(K=1), -1), (dict(K=65), -1), (dict(retain=0), -1), (dict(anchor=2), -1),
                     (dict(tentative=2), -1), (dict(state=odd), -1), (dict(out=odd), -1), (dict(N=33), -3),
                     (dict(Q=1025), -3), (dict(T=513), -3)):
        assert lib.codetr_trail_update_f32(*dict(good, **kw).values()) == code, kw
    rows = (ctypes.c_int64 * 6)(1, 37, 130, 1 + 37 * 130 * 3 + 3, 16, 65)
    size = 1 + 37 * 130 * 3 + 3 + 16 * 65 * 3
    good = dict(stream=None, buf=one, bytes=size, N=2, rows=rows, boxes=one, scores=one, labels=one, count=one, Q=8,
                palette=one, names=one, C=3, lw=3, alpha=0.8, thr=0.3, text=0xc8c8c8, font=1, draw_labels=1, ids=one,
                trails=one, T=2, K=4, tp=one, P=64, tw=2, ta=0.6, color_by=1, show_id=1, untracked=1)
    for kw, code in ((dict(buf=None), -1), (dict(lw=16), -1), (dict(bytes=size - 1), -1), (dict(ids=None), -1),
                     (dict(tp=None), -1), (dict(P=0), -1), (dict(tw=0), -1), (dict(tw=16), -1), (dict(ta=1.5), -1),
                     (dict(ta=float("nan")), -1), (dict(color_by=2), -1), (dict(show_id=2), -1), (dict(untracked=-1), -1),
                     (dict(T=0), -1), (dict(K=1), -1), (dict(K=65), -1), (dict(trails=odd), -1), (dict(T=513), -3),
                     (dict(Q=1025), -3), (dict(P=65537), -3), (dict(N=33), -3), (dict(C=65537), -3),
                     (dict(rows=(ctypes.c_int64 * 6)(1, 37, 130, 100, 16, 65)), -1)):
        assert lib.codetr_draw_tracks_f16(*dict(good, **kw).values()) == code, kw
