"""GPU parity of the fused Swin MLP (C ABI codetr_swin_mlp_{f16,bf16}, csrc/swin_mlp.hip) against a plain PyTorch fp32
reference of the same op, y = x + fc2(gelu(fc1(layer_norm(x)))) (reference codetr/swin.py:331-352), with the tensors the
separate launches would have written -- norm2's output and the hidden activation -- rounded to the storage type between the
steps, and fc2's output rounded before the identity is added.  Tolerance: fp32 accumulation on both sides; the differences are
summation order and which side of a rounding boundary the three intermediate roundings fall: |err| <= 2 ulp of the branch
magnitude + 1 ulp of the result + 2e-3 (3 ulp + 3e-2 for bf16).

Below the line of dashes: both types against the float64 reference of tests/ffn_bounds.py (E(LN(x)), E(gelu(.)), E(W2 h + b2),
E(. + x)), within the bound derived from where the kernel rounds (proved on the CPU by tests/test_ffn_bounds_cpu.py) and with
no more elements off the exact value than 4 x the fp32 emulation's share on the same inputs; guard rows and row isolation.
Row counts come from the device's CU count (walk: 128 (slots + 1) + 45 rows, a second tile walked).  err / bound = 1.000 is an
error of exactly the bound: one step of the storage type.

Largest err / bound and the share of elements that differ from the exact value, measured on MI355X (256 CUs) | the emulation
on the same device, for tails / walk / coherent / offset:
  C = 192  fp16  0.33 / 0.50 / 0.25 / 0.17   0.29 / 0.40 / 0.40 / 0.16 %    |  0.50 / 1.00 / 0.33 / 0.17   0.49 / 0.52 / 0.82 / 0.13 %
           bf16  1.00 / 1.00 / 0.50 / 1.00   0.065 / 0.051 / 0.070 / 0.057 % |  0.50 / 1.00 / 0.50 / 1.00   0.052 / 0.051 / 0.076 / 0.039 %
  C = 384  fp16  0.14 / 0.20 / 0.10 / 0.05   0.80 / 0.69 / 0.70 / 0.16 %    |  0.14 / 0.20 / 0.17 / 0.05   1.10 / 0.91 / 0.96 / 0.12 %
           bf16  0.50 / 1.00 / 0.50 / 0.33   0.023 / 0.072 / 0.098 / 0.066 % |  0.50 / 1.00 / 1.00 / 0.33   0.035 / 0.073 / 0.146 / 0.059 %"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ref(x, g, b, eps, w1, b1, w2, b2):
    dt = x.dtype
    ln = torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), g.float(), b.float(), eps).to(dt).float()
    h = torch.nn.functional.gelu(ln @ w1.float().t() + b1.float()).to(dt).float()
    y = (h @ w2.float().t() + b2.float()).to(dt).float()
    return y + x.float()


def _inputs(M, C, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s, k=1.0: (torch.randn(*s, device=DEV, generator=g) * k).to(dtype)  # noqa: E731
    x = r(M, C, k=1.5) + r(1, C, k=0.5)            # rows with a common offset: the LayerNorm has something to remove
    gam, bet = (1.0 + 0.2 * torch.randn(C, device=DEV, generator=g)).to(dtype), r(C, k=0.2)
    w1, b1 = r(4 * C, C, k=C ** -0.5), r(4 * C, k=0.3)
    w2, b2 = r(C, 4 * C, k=(4 * C) ** -0.5), r(C, k=0.3)
    return x, gam, bet, w1, b1, w2, b2


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 4999, 128 * 256 + 77, 153600])   # tails, one full round + a tail, a whole stage
def test_swin_mlp_vs_fp32(C, M):
    from codetr import _cabi, hip_ops

    x, gam, bet, w1, b1, w2, b2 = _inputs(M, C, torch.float16, seed=M + C)
    before = _cabi.CALLS["swin_mlp"]
    y = hip_ops.swin_mlp(x, gam, bet, 1e-5, w1, b1, w2, b2)
    torch.cuda.synchronize()
    assert _cabi.CALLS["swin_mlp"] == before + 1 and y.shape == x.shape and y.dtype == torch.float16
    ref = _ref(x, gam, bet, 1e-5, w1, b1, w2, b2)
    branch = (ref - x.float()).abs()
    tol = 2.0 ** -10 * (2 * branch + ref.abs()) + 2e-3
    err = (y.float() - ref).abs()
    bad = ~(err <= tol)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} outside; max err {float(err.nan_to_num(1e9).max())}"


@pytest.mark.parametrize("C", [192, 384])
def test_swin_mlp_bf16(C):
    from codetr import hip_ops

    x, gam, bet, w1, b1, w2, b2 = _inputs(40000, C, torch.bfloat16, seed=C)
    y = hip_ops.swin_mlp(x, gam, bet, 1e-5, w1, b1, w2, b2)
    torch.cuda.synchronize()
    ref = _ref(x, gam, bet, 1e-5, w1, b1, w2, b2)
    branch = (ref - x.float()).abs()
    tol = 2.0 ** -7 * (3 * branch + ref.abs()) + 3e-2
    assert ((y.float() - ref).abs() <= tol).all()


def test_repeats_are_bit_identical_and_rows_are_independent():
    """a missed counted wait / an early ring refill shows as a sporadic difference; a row's result must not depend on the tile
    it sits in"""
    from codetr import hip_ops

    x, gam, bet, w1, b1, w2, b2 = _inputs(128 * 300 + 5, 384, torch.float16, seed=9)
    first = hip_ops.swin_mlp(x, gam, bet, 1e-5, w1, b1, w2, b2)
    for _ in range(6):
        assert torch.equal(hip_ops.swin_mlp(x, gam, bet, 1e-5, w1, b1, w2, b2), first)
    shifted = hip_ops.swin_mlp(x[37:].contiguous(), gam, bet, 1e-5, w1, b1, w2, b2)
    assert torch.equal(shifted, first[37:])


def test_swin_block_takes_the_fused_mlp_and_matches_the_separate_launches():
    from codetr import _cabi, hip_ops
    from codetr.swin import SwinBlock

    torch.manual_seed(0)
    blk = SwinBlock(192, 6, 768, window_size=12).to(DEV).half().eval()
    H, W = 192, 180                                   # 34 560 tokens: above SWIN_MLP_MIN_ROWS
    x = torch.randn(1, H * W, 192, device=DEV).half()
    before = dict(_cabi.CALLS)
    with torch.no_grad():
        y = blk(x, (H, W))
    assert _cabi.CALLS["swin_mlp"] == before["swin_mlp"] + 1
    hip_ops.SWIN_MLP = False
    try:
        with torch.no_grad():
            y2 = blk(x, (H, W))
    finally:
        hip_ops.SWIN_MLP = True
    assert _cabi.CALLS["swin_mlp"] == before["swin_mlp"] + 1
    torch.testing.assert_close(y.float(), y2.float(), rtol=2e-3, atol=6e-3)


def test_contract():
    from codetr import _cabi

    lib = _cabi.load()
    assert lib.codetr_swin_mlp_supported(1000, 192, 768) == 1 and lib.codetr_swin_mlp_supported(1000, 384, 1536) == 1
    assert lib.codetr_swin_mlp_supported(1000, 256, 1024) == 0 and lib.codetr_swin_mlp_supported(1000, 192, 512) == 0
    x = torch.zeros(256, 256, dtype=torch.float16, device=DEV)
    st = _cabi.current_stream_ptr(x.device)
    p = x.data_ptr()
    assert lib.codetr_swin_mlp_f16(st, p, p, p, 1e-5, p, p, p, p, p, 256, 256) == -4
    assert lib.codetr_swin_mlp_f16(st, None, p, p, 1e-5, p, p, p, p, p, 256, 192) == -1


# ----------------------------------------------------------------------------------------------------------------------
# float64 interval bounds, tails, a walked second tile (tests/ffn_bounds.py; proved on the CPU by
# tests/test_ffn_bounds_cpu.py), through the _cabi entry that takes the output tensor, which carries GUARD rows of a bit
# pattern behind row M; the row counts come from the device's CU count.
import ffn_bounds as fb  # noqa: E402

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
GUARD, PATTERN = 256, 0x5a5a


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(inp):
    """-> (Y [M, C], None); asserts that the guard rows kept their bits"""
    from codetr import _cabi

    M, C = inp["x"].shape
    y = torch.full((M + GUARD, C), PATTERN, dtype=torch.int16, device=DEV).view(inp["dtype"])
    _cabi.swin_mlp(inp["x"], *inp["ln"], inp["w1"], inp["b1"], _cabi.ffn_pack_w2(inp["w2"].contiguous()), inp["b2"], y)
    torch.cuda.synchronize()
    assert bool((y[M:].view(torch.int16) == PATTERN).all()), "rows behind M were written"
    return y[:M], None


@DTYPES
@pytest.mark.parametrize("name", fb.SWIN_CASE_NAMES)
def test_swin_mlp_within_the_float64_bound_and_share(name, dtype):
    """every element within the derived bound of the float64 reference, and no more elements off the exact value than 4 x
    the emulation's share on the same inputs; the residual is the raw x (every row has an offset of its own)"""
    cus = _cus()
    case = fb.swin_cases(cus)[name]
    for M in case.Ms:
        assert fb.swin_plan(M, case.form, cus).walk == case.walk
    res = fb.measure(case, dtype, _run, DEV, cus)
    print(f"swin {name} {dtype}: err/bound {res.ratio:.3f} (emulated {res.emu_ratio:.3f})  share {res.share:.5f} "
          f"(emulated {res.emu_share:.5f}, cap {fb.share_cap(res):.5f})")
    assert res.ratio <= 1.0
    assert res.share <= fb.share_cap(res)


@DTYPES
@pytest.mark.parametrize("C", [192, 384])
def test_swin_mlp_guard_rows_and_row_isolation(C, dtype):
    """256 rows of a bit pattern behind row M keep their bits at the tail row counts and past a walked second tile; one row set
    to +inf, NaN or 65504 -- row M - 1 of a ragged tile and a row in the middle of a 16-row tile -- leaves every other row the
    bits of the run with that row zeroed"""
    cus = _cus()
    for M in fb.SWIN_TAIL_M + (fb.swin_walk_M(C, cus),):
        y, _ = _run(fb.to_device(fb.swin_random(M, C, dtype), DEV))
        assert bool(torch.isfinite(y).all())
    M = 200
    base = fb.to_device(fb.swin_random(M, C, dtype), DEV)
    for row in (M - 1, 16 * ((M - 1) // 32) + 7):
        keep = torch.arange(M, device=DEV) != row
        zeroed = dict(base, x=base["x"].clone())
        zeroed["x"][row] = 0
        want, _ = _run(zeroed)
        for value in (float("inf"), float("nan"), 65504.0):
            bad = dict(base, x=base["x"].clone())
            bad["x"][row] = value
            got, _ = _run(bad)
            assert torch.equal(got[keep].view(torch.int16), want[keep].view(torch.int16)), (row, value)
