"""CPU: the return code of every rejected call of the 15 tracker entry points -- codetr_track_update_* and
codetr_track_update2_* to 5_*, each in f16, bf16 and f32 -- and with it the ORDER of the argument checks, which one
launcher now performs for all of them: `association` (forms 2 to 5), then the appearance cue's own arguments (form 5, when
desc_dev is given), then the checks every form shares (null pointers and non-positive sizes, sizes too large, non-finite
thresholds, the stream table).  Every call below fails a check, so none reaches a HIP call and no GPU is needed.  The
expected codes were written from the headers' contract and hold for the library before the five kernels, launchers and
forwarding macros became one."""
import ctypes

import pytest

E_BADARG, E_TOO_LARGE = -1, -3
PTR = ctypes.c_void_p(16)        # a device pointer: 16-byte aligned, never dereferenced -- validation fails first
THR = (0.6, 0.1, 0.7, 0.1, 0.5, 0.3)
CUE = (0.75, 0.5, 1.5)           # appearance_thr, proximity_thr, reid_gate
NAN, INF = float("nan"), float("inf")
N, Q, S, T = 2, 300, 2, 256
FORMS = ("", "2", "3", "4", "5")


def _entry(form, suffix):
    from codetr import _appearance, _assign, _cabi, _motion

    lib = {"": _cabi, "2": _assign, "3": _motion, "4": _motion, "5": _appearance}[form].load()
    return getattr(lib, f"codetr_track_update{form}_{suffix}")


def _call(f, form, ptrs=None, N=N, Q=Q, streams=(0, 1), S=S, T=T, settings=THR, retain=30, tentatives=3, association=1,
          motion=PTR, desc=PTR, app_state=PTR, cue=CUE, work=PTR, work_bytes=4 * S * T * Q):
    b, s, l, c, st, out = ptrs or [PTR] * 6
    table = None if streams is None else (ctypes.c_int * len(streams))(*streams)
    values = None if settings is None else (ctypes.c_float * 6)(*settings)
    cue = None if cue is None else (ctypes.c_float * 3)(*cue)
    extras = {"": (), "2": (association,), "3": (association, motion), "4": (association, motion),
              "5": (association, motion, desc, app_state, cue, work, work_bytes)}[form]
    return f(None, b, s, l, c, N, Q, table, S, st, T, values, retain, tentatives, 1, out, *extras)


def _null(i):
    ptrs = [PTR] * 6
    ptrs[i] = None
    return ptrs


def _with(values, i, v):
    return values[:i] + (v,) + values[i + 1:]


# (arguments, the code) for every form; form 5 is called with the cue on (desc_dev given) unless `desc` says otherwise
SHARED = (
    [(dict(ptrs=_null(i)), E_BADARG) for i in range(6)]                 # boxes, scores, labels, count, state, ids_out
    + [(dict(streams=None), E_BADARG), (dict(settings=None), E_BADARG)]
    + [(dict([(k, v)]), E_BADARG) for k in ("N", "Q", "S", "T") for v in (0, -4)]
    + [(dict(N=33, streams=(0,) * 33), E_TOO_LARGE),                     # CODETR_PREPROCESS_BATCH_MAX
       (dict(Q=1025), E_TOO_LARGE),                                      # CODETR_POSTPROCESS_MAX_Q
       (dict(T=513), E_TOO_LARGE),                                       # CODETR_TRACK_MAX_TRACKS
       (dict(S=2 ** 31), E_TOO_LARGE), (dict(N=2 ** 40), E_TOO_LARGE), (dict(T=2 ** 40), E_TOO_LARGE)]
    + [(dict(settings=_with(THR, i, bad)), E_BADARG) for i in range(6) for bad in (NAN, INF, -INF)]
    + [(dict(streams=(0, 2)), E_BADARG), (dict(streams=(-1, 0)), E_BADARG), (dict(streams=(0, 1), S=1), E_BADARG)]
    + [(dict(retain=0), E_BADARG), (dict(retain=-5), E_BADARG), (dict(tentatives=0), E_BADARG),
       (dict(tentatives=-1), E_BADARG)]
    # the order within the shared checks: null and non-positive first, then too large, then thresholds, then the table
    + [(dict(ptrs=_null(0), N=33, streams=(0,) * 33), E_BADARG),
       (dict(retain=0, N=33, streams=(0,) * 33), E_BADARG),
       (dict(N=33, streams=(0,) * 33, settings=_with(THR, 2, NAN)), E_TOO_LARGE),
       (dict(N=33, streams=(9,) * 33), E_TOO_LARGE)])

# forms 2 to 5: association is looked at before anything else
ASSOCIATION = (
    [(dict(association=a), E_BADARG) for a in (-1, 2, 7)]
    + [(dict(association=2, T=513), E_BADARG), (dict(association=2, N=33, streams=(0,) * 33), E_BADARG),
       (dict(association=0, T=513), E_TOO_LARGE), (dict(association=0, ptrs=_null(5)), E_BADARG)])

# form 5: what app_of rejects, after association and before the shared checks; with desc_dev NULL the cue's other
# arguments are not looked at
APPEARANCE = (
    [(dict(desc=ctypes.c_void_p(8)), E_BADARG), (dict(desc=ctypes.c_void_p(17)), E_BADARG),
     (dict(app_state=ctypes.c_void_p(18)), E_BADARG), (dict(work=ctypes.c_void_p(17)), E_BADARG),
     (dict(app_state=None), E_BADARG), (dict(cue=None), E_BADARG), (dict(work=None), E_BADARG)]
    + [(dict(cue=_with(CUE, i, bad)), E_BADARG) for i in (0, 1) for bad in (-0.1, 1.1, NAN, INF, -INF)]
    + [(dict(cue=_with(CUE, 2, bad)), E_BADARG) for bad in (-1.0, NAN, INF, -INF)]
    + [(dict(work_bytes=4 * S * T * Q - 1), E_BADARG), (dict(work_bytes=0), E_BADARG), (dict(work_bytes=-1), E_BADARG),
       # a cue that passes, then a shared check: the cue did not object
       (dict(N=33, streams=(0,) * 33), E_TOO_LARGE),
       (dict(cue=(0.0, 1.0, 0.0), N=33, streams=(0,) * 33), E_TOO_LARGE),
       # the cue's checks come before the shared ones ...
       (dict(work_bytes=4 * S * T * Q - 1, N=33, streams=(0,) * 33), E_BADARG),
       (dict(desc=ctypes.c_void_p(8), N=33, streams=(0,) * 33), E_BADARG),
       (dict(ptrs=_null(0), Q=1025), E_TOO_LARGE),           # ... app_of's "too large" before the shared null check
       (dict(ptrs=_null(0), Q=1025, desc=None), E_BADARG),   # the same call with the cue off: the shared order
       (dict(cue=_with(CUE, 0, NAN), T=513), E_TOO_LARGE),   # within app_of: sizes before settings
       (dict(app_state=None, T=513), E_BADARG),              #                buffers before sizes
       # ... and after association
       (dict(association=2, desc=ctypes.c_void_p(8)), E_BADARG), (dict(association=2, Q=1025), E_BADARG),
       # desc_dev NULL: nothing else of the cue is read
       (dict(desc=None, app_state=None, cue=None, work=None, work_bytes=0, N=33, streams=(0,) * 33), E_TOO_LARGE),
       (dict(desc=None, app_state=ctypes.c_void_p(18), cue=(NAN, NAN, NAN), work_bytes=-1, T=513), E_TOO_LARGE),
       (dict(desc=None, app_state=None, cue=None, work=None, work_bytes=0, retain=0), E_BADARG)])


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("form", FORMS)
def test_track_update_return_codes(form, suffix):
    from codetr import _cabi

    f = _entry(form, suffix)
    table = SHARED + (ASSOCIATION if form else []) + (APPEARANCE if form == "5" else [])
    _cabi.RECORDER = []
    try:
        for association in (0, 1) if form else (1,):
            for kw, want in table:
                kw = dict(dict(association=association), **kw)
                assert _call(f, form, **kw) == want, (form, suffix, kw)
        if form == "5":                                       # every shared case again with the cue off
            for kw, want in SHARED + ASSOCIATION:
                assert _call(f, form, desc=None, **kw) == want, (form, suffix, kw)
        assert _cabi.RECORDER == []                           # no rejected call reached a launch
    finally:
        _cabi.RECORDER = None
