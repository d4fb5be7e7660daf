"""CPU: argument contract of the batched pre- / post-processing entry points (codetr_preprocess_batch_u8_*,
codetr_postprocess_detections_*; include/codetr_hip.h).  Every rejection happens on the host before any HIP call, so
it is checked here without a GPU; the launch recorder proves that nothing was enqueued."""
import ctypes

import pytest

E_BADARG, E_TOO_LARGE = -1, -3


@pytest.fixture
def lib():
    from codetr import _cabi

    _cabi.RECORDER = []
    try:
        yield _cabi.load()
        assert _cabi.RECORDER == []   # no rejected call reached a launch
    finally:
        _cabi.RECORDER = None


def _table(rows):
    return (ctypes.c_int64 * (7 * len(rows)))(*[v for r in rows for v in r])


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_preprocess_batch_rejects_bad_arguments(lib, suffix):
    from codetr import _cabi

    assert _cabi.PREPROCESS_BATCH_MAX == 32
    f = getattr(lib, "codetr_preprocess_batch_u8_" + suffix)
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)
    pad = (ctypes.c_int * 3)(0, 0, 0)
    row = (0, 10, 20, 5, 10, 8, 16)
    ok = dict(src=one, nbytes=600, N=1, tab=_table([row]), H=8, W=16, mean=mean, std=std, pad=pad, dst=one)

    def call(**kw):
        a = dict(ok, **kw)
        return f(None, a["src"], a["nbytes"], a["N"], a["tab"], a["H"], a["W"], a["mean"], a["std"], a["pad"], 0.0,
                 a["dst"], None)

    assert call(src=None) == E_BADARG
    assert call(dst=None) == E_BADARG
    assert call(tab=None) == E_BADARG
    assert call(mean=None) == E_BADARG
    assert call(N=0) == E_BADARG
    assert call(H=0) == E_BADARG
    assert call(N=33, tab=_table([row] * 33)) == E_TOO_LARGE
    assert call(H=65536) == E_TOO_LARGE
    assert call(std=(ctypes.c_float * 3)(1, 0, 1)) == E_BADARG
    assert call(pad=(ctypes.c_int * 3)(0, 256, 0)) == E_BADARG
    assert call(H=7) == E_BADARG                                     # Pad region taller than the batch
    assert call(tab=_table([(0, 10, 20, 9, 10, 8, 16)])) == E_BADARG  # resized image taller than its Pad region
    assert call(nbytes=599) == E_BADARG                              # the image does not lie inside the source buffer
    assert call(tab=_table([(1, 10, 20, 5, 10, 8, 16)])) == E_BADARG
    assert call(tab=_table([(-1, 10, 20, 5, 10, 8, 16)])) == E_BADARG
    assert call(tab=_table([(0, 40000, 1, 5, 10, 8, 16)]), nbytes=120000) == E_TOO_LARGE


@pytest.mark.parametrize("suffix", ["f16", "bf16", "f32"])
def test_postprocess_detections_rejects_bad_arguments(lib, suffix):
    from codetr import _cabi

    assert _cabi.POSTPROCESS_MAX_Q == 1024
    f = getattr(lib, "codetr_postprocess_detections_" + suffix)
    one = ctypes.c_void_p(16)

    def call(ptrs=(one,) * 9, N=2, Q=300):
        b, s, l, d, bo, so, lo, c = ptrs[:8]
        return f(None, b, s, l, d, N, Q, 1, 0.3, 1, 0.8, bo, so, lo, c)

    for i in range(8):
        ptrs = [one] * 8
        ptrs[i] = None
        assert call(ptrs) == E_BADARG, i
    assert call(N=0) == E_BADARG
    assert call(Q=0) == E_BADARG
    assert call(Q=1025) == E_TOO_LARGE
