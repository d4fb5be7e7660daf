"""GPU parity of the token-major GroupNorm (C ABI codetr_groupnorm_tokens_f16) against a plain PyTorch fp32
reference: F.group_norm on the NCHW view of the same data.  Tolerance: 1 fp16 ulp of the output + 2e-3 abs.

Below those: every input family of tests/norm_bounds.py through the real entries, held to the float64 reference within the bound
derived there (tests/test_norm_bounds_cpu.py proves the bound and that the families catch the mutants, fp32 sums of x and x^2
left unchecked among them).  Run with -s for the measured err / bound of every case."""
import pytest
import torch

import norm_bounds as nb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
DT = {F16: "f16", BF16: "bf16"}
BOTH = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
SENTINEL, ROW_START, EXTRA_ROWS = 7.0, 5, 13


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 7, 9), (1, 80, 120), (3, 33, 17), (1, 320, 480)])
def test_groupnorm_tokens_into_slice(B, H, W):
    from codetr import hip_ops

    C, G = 256, 32
    g = torch.Generator(device=DEV).manual_seed(H * W)
    x = (torch.randn(B, H * W, C, device=DEV, generator=g) * 2 + 0.7).half()
    gamma = (1 + 0.2 * torch.randn(C, device=DEV, generator=g)).half()
    beta = (0.3 * torch.randn(C, device=DEV, generator=g)).half()
    S = H * W + 13
    dest = torch.full((B, S, C), 7.0, device=DEV, dtype=torch.float16)
    hip_ops.groupnorm_tokens_into(x, gamma, beta, G, 1e-5, dest, 5)
    torch.cuda.synchronize()
    nchw = x.float().view(B, H, W, C).permute(0, 3, 1, 2)
    ref = torch.nn.functional.group_norm(nchw, G, gamma.float(), beta.float(), 1e-5).permute(0, 2, 3, 1).reshape(B, H * W, C)
    got = dest[:, 5:5 + H * W].float()
    assert ((got - ref).abs() <= 2.0 ** -10 * ref.abs() + 2e-3).all(), float((got - ref).abs().max())
    assert (dest[:, :5] == 7).all() and (dest[:, 5 + H * W:] == 7).all()  # neighbours untouched


def test_groupnorm_tokens_bf16():
    """bf16 storage instantiation against F.group_norm in fp32"""
    import torch.nn.functional as F
    from codetr import _cabi

    g = torch.Generator(device=DEV).manual_seed(4)
    B, HW, C = 2, 777, 256
    x = (torch.randn(B, HW, C, device=DEV, generator=g) * 2 + 0.5).bfloat16()
    gam = (1 + 0.1 * torch.randn(C, device=DEV, generator=g)).bfloat16()
    bet = (0.1 * torch.randn(C, device=DEV, generator=g)).bfloat16()
    out = torch.empty(B, HW + 50, C, dtype=torch.bfloat16, device=DEV)
    _cabi.groupnorm_tokens(x, gam, bet, 32, 1e-5, out[0, 50:], out.shape[1] * C)
    torch.cuda.synchronize()
    ref = F.group_norm(x.float().transpose(1, 2), 32, gam.float(), bet.float(), 1e-5).transpose(1, 2)
    torch.testing.assert_close(out[:, 50:].float(), ref, rtol=1e-2, atol=2e-2)


# ------------------------------------------------------------------------------------------------------- float64 bounds
def _into_slice(x, gamma, beta, groups, through_cabi=False):
    """the kernel's output in a destination slice with sentinel rows on either side, and proof that the native path ran"""
    from codetr import _cabi, hip_ops

    B, HW, C = x.shape
    dest = torch.full((B, HW + EXTRA_ROWS, C), SENTINEL, device=DEV, dtype=x.dtype)
    before = _cabi.CALLS["groupnorm_tokens"]
    if through_cabi:
        _cabi.groupnorm_tokens(x, gamma, beta, groups, 1e-5, dest[0, ROW_START:], dest.shape[1] * C)
    else:
        assert hip_ops.groupnorm_tokens_supported(x, groups)
        hip_ops.groupnorm_tokens_into(x, gamma, beta, groups, 1e-5, dest, ROW_START)
    torch.cuda.synchronize()
    assert _cabi.CALLS["groupnorm_tokens"] == before + 1
    return dest


def _held(what, dest, x, gamma, beta, groups):
    ex = nb.exact_groupnorm_tokens(x, gamma, beta, groups, 1e-5)
    b = nb.bound_groupnorm(ex)
    r = nb.dest_ratio(dest, ROW_START, x.shape[1], SENTINEL, ex, b.total.view(ex.out.shape))
    print(f"{what}: measured err/bound {r:.3f}")
    assert r < 1, (what, r)
    return ex


@BOTH
@pytest.mark.parametrize("groups", nb.GN_GROUPS)
def test_groupnorm_random_inside_float64_bound(groups, dtype):
    """C = 8 .. 2048 (256 .. 1 rows in parallel), token counts around the 128-row slab, three images with their own statistics"""
    for HW in nb.GN_HW:
        x, gamma, beta = nb.gn_random(groups, HW, dtype, DEV)
        _held(f"groupnorm random {DT[dtype]} G{groups} HW{HW}", _into_slice(x, gamma, beta, groups), x, gamma, beta, groups)


@pytest.mark.parametrize("dtype,mean,sigma", [(dt, m, s) for dt in (F16, BF16) for m, s in nb.GN_OFFSET[dt]],
                         ids=[f"{DT[dt]}-{m:g}+-{s:g}" for dt in (F16, BF16) for m, s in nb.GN_OFFSET[dt]])
def test_groupnorm_offset_inside_float64_bound(dtype, mean, sigma):
    """|mean| >> sigma: fp32 sums of x and x^2 lose the variance (rstd wrong by 1e-7 mean^2 / var); the finalize kernel
    notices and the groups' sums are taken again about the first mean"""
    x, gamma, beta = nb.gn_offset(mean, sigma, dtype, DEV)
    dest = _into_slice(x, gamma, beta, 32, through_cabi=True)
    _held(f"groupnorm offset {DT[dtype]} {mean:g}+-{sigma:g}", dest, x, gamma, beta, 32)


@BOTH
def test_groupnorm_outlier_first_token_inside_float64_bound(dtype):
    """token 0 of every image 50 sigma from the mean: the worst input for a pivot taken from token 0"""
    x, gamma, beta = nb.gn_outlier(dtype, DEV)
    _held(f"groupnorm outlier {DT[dtype]}", _into_slice(x, gamma, beta, 32), x, gamma, beta, 32)


@BOTH
def test_groupnorm_constant_image_returns_beta(dtype):
    x, gamma, beta = nb.gn_constant(dtype, DEV)
    dest = _into_slice(x, gamma, beta, 32)
    assert torch.equal(dest[:, ROW_START:ROW_START + x.shape[1]], beta.expand_as(x))
    _held(f"groupnorm constant {DT[dtype]}", dest, x, gamma, beta, 32)


@BOTH
def test_groupnorm_two_valued_group_in_closed_form(dtype):
    """groups m +- d: y = +-gamma d / sqrt(d^2 + eps) + beta, with d^2 of the order of eps"""
    x, gamma, beta = nb.gn_two_valued(dtype, DEV)
    ex = _held(f"groupnorm two_valued {DT[dtype]}", _into_slice(x, gamma, beta, 32), x, gamma, beta, 32)
    assert (ex.out - nb.gn_two_valued_expected(gamma, beta, 1e-5)).abs().max() < 1e-12
