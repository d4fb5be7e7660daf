"""GPU parity of the native LayerNorm (C ABI codetr_layernorm_{f16,bf16}) against a plain PyTorch fp32
reference of the same op.  Tolerance: 1 ulp of the output dtype (single rounding of an fp32 result) +
1e-3 abs for the bf16/fp16 rounding of gamma*xhat near zero.

Below those: every input family of tests/norm_bounds.py through the real entries, held to the float64 reference within the bound
derived there (tests/test_norm_bounds_cpu.py proves the bound and that the families catch the mutants).  Run with -s for the
measured err / bound of every case."""
import pytest
import torch

import norm_bounds as nb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
DT = {F16: "f16", BF16: "bf16"}
BOTH = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,C", [(1, 8), (7, 192), (1000, 256), (513, 384), (300, 768), (77, 1536), (33, 3072),
                                     (5, 4096), (153600, 192), (2, 1000)])
def test_layernorm_vs_fp32(rows, C, dtype):
    from codetr import hip_ops

    g = torch.Generator(device=DEV).manual_seed(rows + C)
    x = (torch.randn(rows, C, device=DEV, generator=g) * 3 + 1.5).to(dtype)
    w = (1 + 0.2 * torch.randn(C, device=DEV, generator=g)).to(dtype)
    b = (0.3 * torch.randn(C, device=DEV, generator=g)).to(dtype)
    y = hip_ops.layer_norm(x, w, b, 1e-5)
    torch.cuda.synchronize()
    ref = torch.nn.functional.layer_norm(x.float(), (C,), w.float(), b.float(), 1e-5)
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    err = (y.float() - ref).abs()
    assert (err <= ulp * ref.abs() + 1e-5 + ulp * 1e-2).all(), float(err.max())
    assert y.dtype == dtype and y.shape == x.shape


def test_layernorm_large_offset_rows_two_pass():
    """rows with |mean| >> std: a one-pass E[x^2]-E[x]^2 formulation loses the variance in fp32."""
    from codetr import hip_ops

    g = torch.Generator(device=DEV).manual_seed(0)
    x = (100.0 + 0.05 * torch.randn(64, 256, device=DEV, generator=g)).half()
    w = torch.ones(256, device=DEV).half()
    b = torch.zeros(256, device=DEV).half()
    y = hip_ops.layer_norm(x, w, b, 1e-5)
    ref = torch.nn.functional.layer_norm(x.float(), (256,), None, None, 1e-5)
    torch.testing.assert_close(y.float(), ref, rtol=2e-3, atol=2e-3)
    ex = nb.exact_layernorm(x, w, b, 1e-5)
    assert nb.ratio(y, ex.out, nb.bound_layernorm(ex).total) < 1


def test_layernorm_3d_and_noncontiguous():
    from codetr import hip_ops

    x = torch.randn(4, 50, 192, device=DEV).half()
    w = torch.randn(192, device=DEV).half()
    b = torch.randn(192, device=DEV).half()
    ref = torch.nn.functional.layer_norm(x.float(), (192,), w.float(), b.float(), 1e-5)
    torch.testing.assert_close(hip_ops.layer_norm(x, w, b).float(), ref, rtol=2e-3, atol=2e-3)
    xt = x.transpose(0, 1)
    torch.testing.assert_close(hip_ops.layer_norm(xt, w, b).float(), ref.transpose(0, 1), rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("B,H,W,C", [(1, 8, 12, 192), (2, 7, 9, 192), (1, 20, 30, 384), (2, 10, 14, 768), (1, 5, 6, 64)])
def test_patch_merge_layernorm_equals_gather_then_layernorm(B, H, W, C):
    """codetr_patch_merge_layernorm_f16 == (2x2 gather in (ky, kx, c) order, zero-padded) -> codetr_layernorm_f16,
    bit for bit (same statistics arithmetic on the same values)."""
    import torch.nn.functional as F
    from codetr import _cabi, hip_ops

    g = torch.Generator(device=DEV).manual_seed(H * 31 + W)
    x = torch.randn(B, H * W, C, device=DEV, generator=g).half()
    gam = (1 + 0.1 * torch.randn(4 * C, device=DEV, generator=g)).half()
    bet = (0.1 * torch.randn(4 * C, device=DEV, generator=g)).half()
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    x4 = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    merged = x4.view(B, H2, 2, W2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H2 * W2, 4 * C)
    ref = hip_ops.layer_norm(merged, gam, bet, 1e-5)
    before = _cabi.CALLS["patch_merge_layernorm"]
    y = hip_ops.patch_merge_layernorm(x, (H, W), gam, bet, 1e-5)      # odd sizes: the kernel pads with zeros itself
    assert _cabi.CALLS["patch_merge_layernorm"] == before + 1
    assert y.shape == ref.shape and torch.equal(y, ref)


def test_patch_merge_layernorm_bf16():
    """bf16 instantiation of the merge + LayerNorm kernel against gather + F.layer_norm in fp32"""
    import torch.nn.functional as F
    from codetr import _cabi

    g = torch.Generator(device=DEV).manual_seed(8)
    B, H, W, C = 2, 14, 10, 96
    x = torch.randn(B, H, W, C, device=DEV, generator=g).bfloat16()
    gam = (1 + 0.1 * torch.randn(4 * C, device=DEV, generator=g)).bfloat16()
    bet = (0.1 * torch.randn(4 * C, device=DEV, generator=g)).bfloat16()
    out = _cabi.patch_merge_layernorm(x, gam, bet, 1e-5)
    torch.cuda.synchronize()
    m = x.float().view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, (H // 2) * (W // 2), 4 * C)
    ref = F.layer_norm(m, (4 * C,), gam.float(), bet.float(), 1e-5)
    torch.testing.assert_close(out.float(), ref, rtol=1e-2, atol=2e-2)


# ------------------------------------------------------------------------------------------------------- float64 bounds
def _layer_norm(x, w, b, eps=1e-5):
    """hip_ops.layer_norm, and proof that the native kernel served it"""
    from codetr import _cabi, hip_ops

    before = _cabi.CALLS["layernorm"]
    y = hip_ops.layer_norm(x, w, b, eps)
    torch.cuda.synchronize()
    assert _cabi.CALLS["layernorm"] == before + 1
    assert y.dtype == x.dtype and y.shape == x.shape
    return y


def _held(what, y, ex):
    r = nb.ratio(y, ex.out, nb.bound_layernorm(ex).total)
    print(f"{what}: measured err/bound {r:.3f}")
    assert r < 1, (what, r)


@BOTH
@pytest.mark.parametrize("C", nb.LN_EDGE_C + nb.LN_MODEL_C)
def test_layernorm_random_inside_float64_bound(C, dtype):
    for rows in nb.LN_ROWS:
        x, w, b = nb.ln_random(rows, C, dtype, DEV)
        _held(f"layernorm random {DT[dtype]} {rows}x{C}", _layer_norm(x, w, b), nb.exact_layernorm(x, w, b, 1e-5))


@BOTH
@pytest.mark.parametrize("rows,C", nb.LN_GRID_STRIDE)
def test_layernorm_grid_stride_inside_float64_bound(rows, C, dtype):
    x, w, b = nb.ln_random(rows, C, dtype, DEV)
    _held(f"layernorm random {DT[dtype]} {rows}x{C}", _layer_norm(x, w, b), nb.exact_layernorm(x, w, b, 1e-5))


@pytest.mark.parametrize("mean,sigma,dtype", nb.LN_OFFSET, ids=[f"{m:g}+-{s:g}-{DT[d]}" for m, s, d in nb.LN_OFFSET])
def test_layernorm_offset_rows_inside_float64_bound(mean, sigma, dtype):
    x, w, b = nb.ln_offset(mean, sigma, dtype, DEV)
    _held(f"layernorm offset {DT[dtype]} {mean:g}+-{sigma:g}", _layer_norm(x, w, b), nb.exact_layernorm(x, w, b, 1e-5))


@BOTH
def test_layernorm_constant_rows_return_beta(dtype):
    """C = 256: every partial sum and the product with 1/256 are exact, x - mean is 0 and y is beta bit for bit;
    C = 192: the rounded 1/192 shows, inside the bound"""
    x, w, b = nb.ln_constant(256, dtype, DEV)
    assert torch.equal(_layer_norm(x, w, b), b.expand_as(x))
    x, w, b = nb.ln_constant(192, dtype, DEV)
    _held(f"layernorm constant {DT[dtype]} C192", _layer_norm(x, w, b), nb.exact_layernorm(x, w, b, 1e-5))


@BOTH
@pytest.mark.parametrize("C", [256, 192])
def test_layernorm_two_valued_rows_in_closed_form(C, dtype):
    """rows m +- d: y = +-gamma d / sqrt(d^2 + eps), with d^2 of the order of eps"""
    x, w, b = nb.ln_two_valued(C, dtype, DEV)
    ex = nb.exact_layernorm(x, w, b, 1e-5)
    assert (ex.out - nb.ln_two_valued_expected(C, w, 1e-5)).abs().max() < 1e-12
    _held(f"layernorm two_valued {DT[dtype]} C{C}", _layer_norm(x, w, b), ex)


@BOTH
@pytest.mark.parametrize("C", nb.LN_LAST_CHUNK_C)
def test_layernorm_last_chunk_alone_non_zero(C, dtype):
    """zeros but for the last 16-byte chunk: every zero returns -mean rstd gamma + beta, in closed form"""
    x, w, b = nb.ln_last_chunk(C, dtype, DEV)
    ex = nb.exact_layernorm(x, w, b, 1e-5)
    assert (ex.out - nb.ln_last_chunk_expected(x, w, b, 1e-5)).abs().max() < 1e-12
    _held(f"layernorm last_chunk {DT[dtype]} C{C}", _layer_norm(x, w, b), ex)


@BOTH
@pytest.mark.parametrize("rows,C", [(33, 192), (33, 1032), (33, 4096), nb.LN_GRID_STRIDE[0]])
def test_layernorm_in_place(rows, C, dtype):
    """y may alias x (include/codetr_hip.h): a lane holds its part of the row in registers before it stores"""
    from codetr import _cabi

    x, w, b = nb.ln_random(rows, C, dtype, DEV)
    ex = nb.exact_layernorm(x, w, b, 1e-5)
    apart = _cabi.layernorm(x, w, b, 1e-5, torch.empty_like(x))
    buf = x.clone()
    before = _cabi.CALLS["layernorm"]
    _cabi.layernorm(buf, w, b, 1e-5, buf)
    torch.cuda.synchronize()
    assert _cabi.CALLS["layernorm"] == before + 1
    assert torch.equal(buf, apart)
    _held(f"layernorm in place {DT[dtype]} {rows}x{C}", buf, ex)


@BOTH
@pytest.mark.parametrize("B,H,W,Cs", nb.MERGE_SHAPES)
def test_patch_merge_layernorm_inside_float64_bound_and_equal_to_gather_then_layernorm(B, H, W, Cs, dtype):
    """every source pixel has its own statistics: a mis-routed gather leaves the bound by orders of magnitude.  The kernel still
    equals gather -> codetr_layernorm bit for bit, in both types and at the smallest shapes."""
    from codetr import _cabi, hip_ops

    x, w, b = nb.merge_input(B, H, W, Cs, dtype, DEV)
    ex = nb.exact_patch_merge_layernorm(x, w, b, 1e-5)
    before = _cabi.CALLS["patch_merge_layernorm"]
    y = hip_ops.patch_merge_layernorm(x.view(B, H * W, Cs), (H, W), w, b, 1e-5)
    y2 = _cabi.patch_merge_layernorm(x, w, b, 1e-5)
    torch.cuda.synchronize()
    assert _cabi.CALLS["patch_merge_layernorm"] == before + 2
    assert y.dtype == dtype and y.shape == ex.out.shape and torch.equal(y, y2)
    _held(f"patch merge {DT[dtype]} {B}x{H}x{W}x{Cs}", y, ex)
    assert torch.equal(y, _layer_norm(nb.exact_patch_merge(x), w, b))
