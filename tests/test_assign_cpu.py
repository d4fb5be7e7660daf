"""CPU: the assignment procedure of include/codetr_assign.h -- its numpy restatement (tests/assign_ref.py) against
scipy's optimum, the header and its binding, the argument contract of the new entry points, how `association=` and
`track_association=` are read, and the crossing case that greedy loses, worked through both tracker restatements.  The
kernels are compared with the restatements element for element in test_assign_gpu.py."""
import ctypes
import glob
import os

import numpy as np
import pytest

import assign_ref
from conftest import ROOT
from track_assign_ref import TrackAssignRef, gains
from track_ref import F, TrackRef

E_BADARG, E_TOO_LARGE = -1, -3
SWIN = glob.glob(os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py"))[0]
GMAX = assign_ref.MAX_GAIN


def _inferencer(**kw):
    from codetr.inferencer import Inferencer

    return Inferencer(None, SWIN, dataset_meta=None, **kw)


# ---- 1. the restatement is optimal -------------------------------------------------------------------------------------
def random_gains(rng, n, m, density=1.0, hi=GMAX):
    G = rng.integers(1, hi + 1, (n, m))
    if density < 1.0:
        G = G * (rng.random((n, m)) < density)
    return G.astype(np.int64)


def _check(G):
    match, total, rounds = assign_ref.solve(G)
    assert assign_ref.check_matching(G, match) == total       # a valid matching, every matched pair of positive gain
    assert total == assign_ref.optimum(G)                      # exactly scipy's optimum
    n, m = np.asarray(G).shape
    assert n <= rounds <= n * (max(n, m) + 1)
    return match, total, rounds


@pytest.mark.parametrize("shape", ["n<m", "n==m", "n>m"])
@pytest.mark.parametrize("density", [1.0, 0.05, 0.02])
def test_random_matrices_reach_scipys_optimum(shape, density):
    rng = np.random.default_rng(int(density * 1000) + len(shape))
    for k in range(40):
        a, b = sorted(int(v) for v in rng.integers(1, 48, 2))
        n, m = {"n<m": (a, b + 1), "n==m": (b, b), "n>m": (b + 1, a)}[shape]
        hi = (3, 50, GMAX)[k % 3]                              # small ranges tie often
        _check(random_gains(rng, n, m, density, hi))


def test_structured_matrices():
    for n in (1, 2, 7, 33):
        m, total, rounds = _check(np.full((n, n), 5))
        assert m.tolist() == list(range(n)) and rounds == n * (n + 1) // 2     # row i walks the i columns held before it
        m, total, _ = _check(np.outer(np.arange(1, n + 1), np.arange(1, n + 1)))
        assert m.tolist() == list(range(n)) and total == sum(k * k for k in range(1, n + 1))
        m, total, _ = _check(np.zeros((n, n + 2), np.int64))
        assert (m == -1).all() and total == 0
    rng = np.random.default_rng(5)
    G = random_gains(rng, 12, 9)
    G[[0, 5, 11]] = 0                                           # zero rows stay unmatched
    m, _, _ = _check(G)
    assert m[0] == m[5] == m[11] == -1 and (m >= 0).sum() == 9
    G = random_gains(rng, 6, 6)
    G[:, 2] = 0                                                 # a zero column is never reported
    assert 2 not in _check(G)[0].tolist()


def test_gains_are_clamped():
    G = np.array([[-5, 3], [2 ** 30, 2 ** 30]])
    m, total, _ = assign_ref.solve(G)
    assert total == 3 + GMAX and m.tolist() == [1, 0]


def test_the_issues_example():
    """values [[0.60, 0.55], [0.58, 0.05]] at threshold 0.1: greedy takes 0.60 and leaves row 1 nothing; the assignment
    takes 0.55 + 0.58"""
    val = np.array([[0.60, 0.55], [0.58, 0.05]], np.float32)
    g = gains(val, F(0.1))
    assert g[1, 1] == 0 and g[0, 0] == 1 + int((F(0.60) - F(0.1)) * F(1048576.0))
    m, total, _ = _check(g)
    assert m.tolist() == [1, 0] and total == g[0, 1] + g[1, 0]
    assert gains(np.array([np.nan, 0.1, 5.0, np.inf], np.float32), F(0.1)).tolist() == [0, 1, GMAX, GMAX]


# ---- 2. the header and its binding -------------------------------------------------------------------------------------
def test_header_parses_and_the_table_equals_its_declarations():
    from codetr import _assign, _cabi, _cheader

    text = open(os.path.join(ROOT, "include", "codetr_assign.h")).read()
    functions, defines = _cheader.parse(text)
    assert list(functions) == ["codetr_assign_abi_version", "codetr_assign_i32", "codetr_track_update2_f16",
                               "codetr_track_update2_bf16", "codetr_track_update2_f32"]
    assert defines == dict(CODETR_ASSIGN_ABI_VERSION=1, CODETR_ASSIGN_MAX_ROWS=512, CODETR_ASSIGN_MAX_COLS=1024,
                           CODETR_ASSIGN_MAX_GAIN=2 ** 21 + 1, CODETR_ASSOCIATION_GREEDY=0, CODETR_ASSOCIATION_OPTIMAL=1)
    assert _assign.MAX_GAIN == GMAX == 1 + 2 * 1048576
    assert set(_assign.SIGNATURES) == set(functions)
    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _assign.SIGNATURES["codetr_assign_abi_version"] == (i, [])
    assert _assign.SIGNATURES["codetr_assign_i32"] == (i, [p, p, l, l, l, p, p])
    old = _cabi.SIGNATURES["codetr_track_update_f16"]
    for suffix in ("f16", "bf16", "f32"):                      # the old entry's arguments + int association
        assert _assign.SIGNATURES["codetr_track_update2_" + suffix] == (old[0], old[1] + [i])
        ret, params = functions["codetr_track_update2_" + suffix]
        assert [n for _, n in params[:-1]] == [n for _, n in _cheader.functions["codetr_track_update_" + suffix][1]]
        assert params[-1] == ("int", "association")
    assert not set(functions) & set(_cabi.SIGNATURES)           # a companion: codetr_hip.h and its version are untouched
    for phrase in ("ties to the lowest column index", "parity\n *   stays unpinned", "1 + (int)(fminf(value - thr, 2.0f) * 1048576.0f)"):
        assert phrase in text, phrase


@pytest.fixture
def lib():
    from codetr import _assign, _cabi

    _cabi.RECORDER = []
    try:
        yield _assign.load()
        assert _cabi.RECORDER == []
    finally:
        _cabi.RECORDER = None


def test_abi_version(lib):
    from codetr import _assign

    assert _assign.ABI_VERSION == 1 and lib.codetr_assign_abi_version() == 1
    assert lib.codetr_hip_abi_version() == 54


def test_assign_rejects_bad_arguments(lib):
    one = ctypes.c_void_p(16)   # device pointers: never dereferenced, validation fails first

    def call(ptrs=None, B=2, n=5, m=7):
        g, mt, tot = ptrs or [one] * 3
        return lib.codetr_assign_i32(None, g, B, n, m, mt, tot)

    for k in range(3):
        ptrs = [one] * 3
        ptrs[k] = None
        assert call(ptrs) == E_BADARG, k
    for name in ("B", "n", "m"):
        assert call(**{name: 0}) == E_BADARG and call(**{name: -3}) == E_BADARG, name
    assert call(n=513) == E_TOO_LARGE and call(m=1025) == E_TOO_LARGE and call(B=65536) == E_TOO_LARGE
    assert call(n=2 ** 40) == E_TOO_LARGE


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_track_update2_rejects_bad_arguments(lib, suffix):
    f = getattr(lib, "codetr_track_update2_" + suffix)
    one = ctypes.c_void_p(16)
    thr = (0.6, 0.1, 0.7, 0.1, 0.5, 0.3)

    def call(ptrs=None, N=2, Q=300, streams=(0, 1), S=2, T=256, settings=thr, retain=30, tentatives=3, association=1):
        b, s, l, c, st, out = ptrs or [one] * 6
        table = None if streams is None else (ctypes.c_int * len(streams))(*streams)
        values = None if settings is None else (ctypes.c_float * 6)(*settings)
        return f(None, b, s, l, c, N, Q, table, S, st, T, values, retain, tentatives, 1, out, association)

    for association in (0, 1):
        for i in range(6):
            ptrs = [one] * 6
            ptrs[i] = None
            assert call(ptrs, association=association) == E_BADARG, i
        assert call(streams=None, association=association) == E_BADARG
        assert call(settings=None, association=association) == E_BADARG
        for name in ("N", "Q", "S", "T"):
            assert call(**{name: 0}, association=association) == E_BADARG, name
        assert call(streams=(0, 2), association=association) == E_BADARG
        assert call(settings=thr[:2] + (float("nan"),) + thr[3:], association=association) == E_BADARG
        assert call(retain=0, association=association) == E_BADARG and call(tentatives=0, association=association) == E_BADARG
        assert call(N=33, streams=(0,) * 33, association=association) == E_TOO_LARGE
        assert call(Q=1025, association=association) == E_TOO_LARGE
        assert call(T=513, association=association) == E_TOO_LARGE
    for association in (-1, 2, 7):
        assert call(association=association) == E_BADARG


# ---- 3. Python arguments -----------------------------------------------------------------------------------------------
def test_python_argument_validation():
    import torch
    from codetr import hip_ops
    from codetr.inferencer import track_association_setting

    assert hip_ops.TRACK_ASSOCIATIONS == ("greedy", "optimal")
    for bad in ("hungarian", "", None, 1, True):
        with pytest.raises(ValueError, match="association"):
            hip_ops.track_update(None, None, association=bad)   # read before anything else is touched
    for bad in (torch.zeros((2, 2), dtype=torch.int64), torch.zeros((2,), dtype=torch.int32),
                torch.zeros((1, 1, 2, 2), dtype=torch.int32), np.zeros((2, 2), np.int32),
                torch.zeros((513, 4), dtype=torch.int32), torch.zeros((2, 4, 1025), dtype=torch.int32)):
        with pytest.raises(ValueError, match="linear_assignment"):
            hip_ops.linear_assignment(bad)
    with pytest.raises(RuntimeError, match="MI355X only"):      # no CPU fallback behind it
        hip_ops.linear_assignment(torch.zeros((2, 2), dtype=torch.int32))

    assert track_association_setting(None, None) == "greedy" == track_association_setting(None, {})
    assert _inferencer().track_association == "greedy" and _inferencer().tracker is None
    assert _inferencer(tracker={}).track_association == "greedy"
    assert _inferencer(tracker={}, track_association="greedy").track_association == "greedy"
    assert _inferencer(tracker={}, track_association="optimal").track_association == "optimal"
    for bad in ("lap", 1, True, dict(type="optimal")):
        with pytest.raises(ValueError, match="track_association"):
            _inferencer(tracker={}, track_association=bad)
    for name in ("greedy", "optimal"):
        with pytest.raises(ValueError, match="without a tracker"):
            _inferencer(track_association=name)
    with pytest.raises(ValueError):                              # still no key of the tracker dict
        _inferencer(tracker=dict(association="optimal"))


# ---- 4. the crossing case ----------------------------------------------------------------------------------------------
def test_crossing_keeps_both_ids_only_under_the_assignment():
    """crossing_case (track_assign_cases.py): tracks 1 and 2, then one frame in which track 1's best pair is also track
    2's only pair above the threshold.  Greedy gives it to track 1: track 2 is lost and its detection starts id 3.  The
    assignment gives track 1 its second choice and keeps both."""
    import track_assign_cases as cases

    b, s, l, c = cases.crossing_case()
    vals = cases.crossing_values()
    assert vals[0, 0] > vals[1, 0] > vals[0, 1] > 0.1 > vals[1, 1] and vals[0, 1] + vals[1, 0] > vals[0, 0]
    greedy, optimal = TrackRef(), TrackAssignRef()
    ids_g = [greedy.update(b[f], s[f], l[f], c[f]).tolist() for f in range(len(c))]
    ids_o = [optimal.update(b[f], s[f], l[f], c[f]).tolist() for f in range(len(c))]
    assert ids_g[0] == ids_o[0] == [1, 2]
    assert ids_g[1] == [1, -3] and greedy.state().next_id == 4          # an identity switch
    assert ids_o[1] == [2, 1] and optimal.state().next_id == 3          # both ids persist
    assert ids_o[2] == [2, 1]
    assert optimal.log["A"] == 4 and optimal.log["problems"] == 2 and optimal.log["rounds"] >= 4
