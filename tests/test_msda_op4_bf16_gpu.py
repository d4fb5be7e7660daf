"""The bf16 form of the windowed kernel behind the public op for encoder-shaped calls (csrc/msda_op4.hip,
codetr_msda_op4_forward_bf16) against the C / fp64 oracle (oracle/msda_ref.c: reference ms_deform_attn.cu:31-77, 211-261),
THROUGH torch.ops.codetr.multi_scale_deformable_attention and through its own C-ABI entry.  The bf16 mirror of
tests/test_msda_op4_gpu.py.

Tolerance: one bf16 ulp (2^-7 relative at most) of the exactly computed result plus fp32 accumulation noise -- the kernel
widens bf16 exactly, blends in fp32 and rounds once to nearest even; and, element by element, the output is at most one bf16
ulp away from the oracle's result rounded to bf16 (where the two differ by more than the fp32 noise floor: a result that
cancels to almost zero has ulps far below that noise).

The host-only checks at the end need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import msda_oracle as O

DEV = "cuda:0"
M, L, P, D = 8, 5, 4, 32
PYR_608 = [(76, 76), (38, 38), (19, 19), (10, 10), (5, 5)]
PYR_DIV = [(64, 96), (32, 48), (16, 24), (8, 12), (4, 6)]
PYR_ODD = [(77, 51), (39, 26), (20, 13), (10, 7), (5, 4)]
RTOL, ATOL = 1.1 * 2.0 ** -7, 2e-6


def _bf(a):
    """float64 array -> the nearest bf16 values, as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float().to(torch.bfloat16).double().numpy()


def _tensors(shapes):
    ss = np.asarray(shapes, dtype=np.int64)
    ls = np.concatenate(([0], np.cumsum(ss[:, 0] * ss[:, 1])[:-1])).astype(np.int64)
    return ss, ls, int((ss[:, 0] * ss[:, 1]).sum())


def _case(shapes, B, spread_px, seed, mode="pixel"):
    """value, loc, w as bf16-representable float64 arrays.  mode 'pixel': query i sits at pixel i of the pyramid and samples
    around its own position (spread in pixels of each level); 'uniform': locations anywhere in [-0.1, 1.1]"""
    ss, ls, S = _tensors(shapes)
    rng = np.random.default_rng(seed)
    value = rng.standard_normal((B, S, M, D))
    w = rng.random((B, S, M, L, P))
    w = w / w.sum((-1, -2), keepdims=True) * rng.uniform(0.5, 2.0, (B, S, M, 1, 1))   # not normalised: the op must not care
    if mode == "uniform":
        loc = rng.uniform(-0.1, 1.1, (B, S, M, L, P, 2))
    else:
        centres = []
        for (h, w_) in shapes:
            ys, xs = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w_) + 0.5) / w_, indexing="ij")
            centres.append(np.stack((xs.ravel(), ys.ravel()), -1))
        c = np.concatenate(centres, 0)                                   # [S, 2] normalised (x, y)
        size = np.asarray([[w_, h] for h, w_ in shapes], dtype=np.float64)  # [L, 2] (W, H)
        off = rng.standard_normal((B, S, M, L, P, 2)) * spread_px
        loc = c[None, :, None, None, None, :] + off / size[None, None, None, :, None, :]
    return _bf(value), ss, ls, _bf(loc), _bf(w), S


def _expect(value, ss, ls, loc, w):
    return O.msda_forward_c(value, ss, ls, loc, w, dtype=np.float64)


def _dev(a, dt):
    return torch.as_tensor(np.asarray(a)).to(DEV).to(dt).contiguous()


def _op(value, ss, ls, loc, w):
    import codetr  # noqa: F401

    out = torch.ops.codetr.multi_scale_deformable_attention(_dev(value, torch.bfloat16), _dev(ss, torch.int64), _dev(ls, torch.int64),
                                                            _dev(loc, torch.bfloat16), _dev(w, torch.bfloat16), 64)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16
    return out.float().cpu().numpy()


def _direct(value, ss, ls, loc, w):
    """the windowed kernel alone on a NaN-filled output: (rc, output)"""
    from codetr import _cabi

    lib = _cabi.load()
    v, s_, l_ = _dev(value, torch.bfloat16), _dev(ss, torch.int64), _dev(ls, torch.int64)
    lo, we = _dev(loc, torch.bfloat16), _dev(w, torch.bfloat16)
    B, S = v.shape[:2]
    out = torch.full((B, S, M * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.codetr_msda_op4_forward_bf16(_cabi.current_stream_ptr(v.device), v.data_ptr(), s_.data_ptr(), l_.data_ptr(),
                                          lo.data_ptr(), we.data_ptr(), B, S, M, D, L, S, P, out.data_ptr())
    torch.cuda.synchronize()
    return rc, out.float().cpu().numpy()


def _ordered(x):
    """bf16 values (as float) -> integers in the order of the values: adjacent bf16 numbers differ by 1"""
    bits = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).int().numpy()
    mag = bits & 0x7FFF
    return np.where(bits < 0, -mag, mag).astype(np.int64)


def _check(got, ref, what):
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} outputs not written / not finite"
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=what)
    ulps = np.abs(_ordered(got) - _ordered(_bf(ref)))
    far = (ulps > 1) & (np.abs(got - ref) > ATOL)
    assert not far.any(), f"{what}: {int(far.sum())} outputs more than one bf16 ulp from the rounded oracle (max {int(ulps[far].max())})"


@pytest.mark.gpu
@pytest.mark.parametrize("shapes", [PYR_608, PYR_DIV, PYR_ODD], ids=["608", "divisible", "odd"])
@pytest.mark.parametrize("spread", [1.5, 6.0, 40.0], ids=["inside", "beyond_window", "outside_image"])
def test_windowed_kernel_alone_vs_oracle(shapes, spread):
    value, ss, ls, loc, w, S = _case(shapes, 2, spread, seed=int(spread * 10) + len(shapes[0]))
    rc, got = _direct(value, ss, ls, loc, w)
    assert rc == 0
    _check(got, _expect(value, ss, ls, loc, w), f"spread {spread}")


@pytest.mark.gpu
def test_uniform_locations_and_non_finite_through_the_op():
    value, ss, ls, loc, w, S = _case(PYR_608, 1, 0.0, seed=3, mode="uniform")
    loc[0, 5, 1, 2, 3, 0] = np.nan
    loc[0, 77, 0, 0, 0, 1] = np.inf
    loc[0, 1234, 7, 4, 1, :] = -np.inf
    got = _op(value, ss, ls, loc, w)
    ref = _expect(value, ss, ls, np.nan_to_num(loc, nan=-1e4, posinf=1e4, neginf=-1e4), w)   # all dropped by the reference's gate
    _check(got, ref, "uniform + non-finite")
    rc, alone = _direct(value, ss, ls, loc, w)
    assert rc == 0
    np.testing.assert_array_equal(alone, got)          # the op's bf16 result IS the windowed kernel's


@pytest.mark.gpu
def test_plan_turns_down_odd_pyramids_and_the_general_kernel_serves_them():
    # level 0 is not the largest level: the windowed kernel's workgroups must return without touching `out`
    shapes = [(19, 19), (76, 76), (38, 38), (10, 10), (5, 5)]
    value, ss, ls, loc, w, S = _case(shapes, 1, 0.0, seed=4, mode="uniform")
    rc, alone = _direct(value, ss, ls, loc, w)
    assert rc == 0 and np.isnan(alone).all()
    _check(_op(value, ss, ls, loc, w), _expect(value, ss, ls, loc, w), "turned-down pyramid through the op")
    # level starts that are not the prefix sums (a padded layout): same
    value, ss, ls, loc, w, S = _case(PYR_608, 1, 2.0, seed=5)
    ls2 = ls.copy()
    ls2[1:] = ls[1:][::-1].copy()
    rc, alone = _direct(value, ss, ls2, loc, w)
    assert rc == 0 and np.isnan(alone).all()


@pytest.mark.gpu
def test_full_size_matches_the_fp32_op():
    """BASELINE's pyramid (S = 204 600), model-like locations: the bf16 op against the fp32 op (the general kernel) on the
    same bf16 inputs, its result rounded to bf16: within one bf16 ulp"""
    shapes = [(320, 480), (160, 240), (80, 120), (40, 60), (20, 30)]
    ss, ls, S = _tensors(shapes)
    g = torch.Generator(device=DEV).manual_seed(1)
    value = torch.randn(1, S, M, D, device=DEV, generator=g).bfloat16()
    cs = []
    for (h, w_) in shapes:
        ys, xs = torch.meshgrid((torch.arange(h, device=DEV) + 0.5) / h, (torch.arange(w_, device=DEV) + 0.5) / w_, indexing="ij")
        cs.append(torch.stack((xs.reshape(-1), ys.reshape(-1)), -1))
    c = torch.cat(cs, 0)
    size = torch.tensor([[w_, h] for h, w_ in shapes], device=DEV, dtype=torch.float32)
    off = torch.randn(1, S, M, L, P, 2, device=DEV, generator=g) * 3.0
    loc = (c[None, :, None, None, None, :] + off / size[None, None, None, :, None, :]).bfloat16()
    w = torch.softmax(torch.randn(1, S, M, L * P, device=DEV, generator=g), -1).view(1, S, M, L, P).bfloat16()
    sst, lst = torch.as_tensor(ss).to(DEV), torch.as_tensor(ls).to(DEV)
    import codetr  # noqa: F401
    from codetr import _cabi

    got = torch.ops.codetr.multi_scale_deformable_attention(value, sst, lst, loc, w, 64)
    ref = torch.ops.codetr.multi_scale_deformable_attention(value.float(), sst, lst, loc.float(), w.float(), 64)
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and torch.isfinite(got.float()).all()
    gotn, refn = got.float().cpu().numpy(), ref.cpu().numpy()
    np.testing.assert_allclose(gotn, refn, rtol=RTOL, atol=1e-5)
    ulps = np.abs(_ordered(gotn) - _ordered(refn))
    far = (ulps > 1) & (np.abs(gotn - refn) > 1e-5)
    assert not far.any(), f"{int(far.sum())} outputs more than one bf16 ulp from the fp32 op's result"
    assert _cabi.load().codetr_msda_op4_supported(2, 1, S, M, D, L, S, P) == 1


def test_bf16_entry_is_exported_and_checks_its_arguments_on_the_host():
    """No GPU needed: the argument checks run before anything is launched"""
    from codetr import _cabi

    lib = _cabi.load()
    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), "codetr_msda_op4_forward_bf16")
    f = lib.codetr_msda_op4_forward_bf16
    one = ctypes.c_void_p(16)   # (never dereferenced: every call below is turned down first)
    S = 7725
    assert f(None, None, one, one, one, one, 2, S, M, D, L, S, P, one) == -1              # CODETR_E_BADARG
    assert f(None, one, one, one, one, one, 2, S, M, D, L, 900, P, one) == _cabi.E_UNSUPPORTED   # decoder-shaped
    assert f(None, one, one, one, one, one, 2, S, M, 64, L, S, P, one) == _cabi.E_UNSUPPORTED    # 64-channel heads
    assert f(None, one, one, one, one, one, 2, 512, M, D, L, 512, P, one) == _cabi.E_UNSUPPORTED  # launch-bound sizes
    assert f(None, one, one, one, one, ctypes.c_void_p(20), 2, S, M, D, L, S, P, one) == _cabi.E_UNSUPPORTED   # weight alignment
