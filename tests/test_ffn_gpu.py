"""GPU parity of the fused FFN kernel (C ABI codetr_ffn_relu_f16) against a plain PyTorch fp32 reference of the
same op, y = x + relu(x W1^T + b1) W2^T + b2, with the hidden activation rounded to fp16 between the products (what
the kernel -- and the reference's fp16 path -- does).  Tolerance: fp32 accumulation on both sides; differences are
summation order + the two fp16 roundings of the FFN branch: |err| <= 2 ulp(fp16) of the branch magnitude + 1 ulp
of the result.

Below the line of dashes: every form and both types against the float64 reference of tests/ffn_bounds.py, within the bound
derived from where the kernel rounds (proved on the CPU by tests/test_ffn_bounds_cpu.py) and with no more elements off the
exact value than 4 x the fp32 emulation's share on the same inputs; exact small-integer cases (bit equality); guard rows, row
isolation, one row one result.  Row counts come from the device's CU count (tails: the 64-row form alone; ragged: the 128-row
form alone; multi: a second tile walked; split: both launches).  err / bound = 1.000 is an error of exactly the bound: one step
of the storage type where the interval straddles one rounding boundary.  The oproj bounds are wide (three products and two
norms widen the interval; in bf16 many rows are promised nothing): those forms are held by the share and by the exact cases.

Largest err / bound per form, and the share of elements that differ from the exact value, measured on MI355X (256 CUs) | the
emulation on the same device:
                                 fp16 err/bound   share              bf16 err/bound   share
  plain    tails h64 / h2048     1.00 / 0.25      0.008 % / 0.34 %   1.00 / 1.00      0.001 % / 0.021 %
           emulated              1.00 / 0.25      0.081 % / 0.65 %   1.00 / 1.00      0.001 % / 0.026 %
  plain    ragged, multi h64-192 0.50, 1.00       0.30 %, 0.06-0.11 %   1.00, 1.00    0.034 %, 0.005-0.009 %
           emulated              0.50, 1.00       0.63 %, 0.10-0.22 %   1.00, 1.00    0.027 %, 0.007-0.010 %
  full     tails h64 / h2048     0.50 / 0.10      0.47 % / 0.63 %    1.00 / 0.33      0.057 % / 0.044 %
           emulated              0.50 / 0.11      0.19 % / 1.10 %    1.00 / 0.33      0.083 % / 0.035 %
  full     ragged, split         0.14, 0.17       0.72 %, 0.77 %     0.50, 1.00       0.080 %, 0.082 %
           emulated              0.17, 0.17       1.13 %, 1.16 %     1.00, 0.50       0.076 %, 0.080 %
  oproj    multi h64-192, split  0.02-0.05, 0.004 0.47-0.60 %, 0.97 %   <= 0.04, 0.00 0.045-0.066 %, 0.097 %
           emulated              0.02-0.04, 0.004 0.75-0.97 %, 1.72 %   <= 0.04, 0.00 0.043-0.062 %, 0.109 %
  distinct norms, 200 / ragged   0.90 / 1.00      0.27 % / 0.048 %   0.01 / 1.00      0.002 % / 0.004 %
           emulated              0.90 / 0.89      0.26 % / 0.039 %   0.00 / 1.00      0.000 % / 0.002 %
  coherent h64 / h512            1.00 / 0.40      0.20 % / 0.27 %    0.00 / 1.00      0.000 % / 0.025 %
           emulated              1.00 / 0.50      0.12 % / 0.65 %    0.00 / 1.00      0.000 % / 0.037 %
With the hidden pack of ffn_fused.hip changed to truncate (not committed), every one of these cases fails in both types --
the hidden = 64 and the coherent cases outside the bound, with 40 % / 92 % / 99.9 % of the elements off the exact value, the
shares the CPU emulation of that mutant gives -- and the exact-integer cases still pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ref(x, w1, b1, w2, b2):
    h = torch.relu(x.float() @ w1.float().t() + b1.float()).half().float()
    y = (h @ w2.float().t() + b2.float()).half().float()
    return (y + x.float())


@pytest.mark.parametrize("M,hidden", [(1, 64), (128, 2048), (129, 2048), (900, 2048), (5000, 512), (30785, 2048),
                                      (128 * 256 + 4999, 256)])  # one full round of 256 tiles + a tail of 64-row tiles
def test_ffn_fused_vs_fp32(M, hidden):
    from codetr import _cabi, hip_ops

    g = torch.Generator(device=DEV).manual_seed(M + hidden)
    x = torch.randn(M, 256, device=DEV, generator=g).half()
    w1 = (torch.randn(hidden, 256, device=DEV, generator=g) / 16).half()
    b1 = (torch.randn(hidden, device=DEV, generator=g) * 0.5).half()
    w2 = (torch.randn(256, hidden, device=DEV, generator=g) / hidden ** 0.5).half()
    b2 = (torch.randn(256, device=DEV, generator=g) * 0.5).half()
    before = _cabi.CALLS["ffn_fused"]
    y = hip_ops.ffn_fused(x, w1, b1, w2, b2)
    torch.cuda.synchronize()
    assert _cabi.CALLS["ffn_fused"] == before + 1 and y.shape == x.shape and y.dtype == torch.float16
    ref = _ref(x, w1, b1, w2, b2)
    branch = (ref - x.float()).abs()
    tol = 2.0 ** -10 * (2 * branch + ref.abs()) + 2e-3
    err = (y.float() - ref).abs()
    assert (err <= tol).all(), f"max err {float(err.max())} at tol {float(tol.flatten()[err.argmax()])}"


def test_ffn_module_takes_fused_path_and_matches_two_gemm_path():
    from codetr import _cabi, hip_ops
    from codetr.transformer_layers import FFN

    torch.manual_seed(0)
    ffn = FFN(embed_dims=256, feedforward_channels=2048).to(DEV).half().eval()
    x = torch.randn(2, hip_ops.FFN_FUSED_MIN_ROWS // 2 + 77, 256, device=DEV).half()
    before = dict(_cabi.CALLS)
    with torch.no_grad():
        y = ffn(x)
        fc1, fc2 = ffn.layers[0][0], ffn.layers[1]
        h = hip_ops.linear(x, fc1.weight, fc1.bias, act="relu")
        y2 = hip_ops.linear(h, fc2.weight, fc2.bias, residual=x)
    assert _cabi.CALLS["ffn_fused"] == before["ffn_fused"] + 1
    torch.testing.assert_close(y.float(), y2.float(), rtol=2e-3, atol=4e-3)
    # explicit identity / no identity keep the two-GEMM path (different residual semantics)
    with torch.no_grad():
        y3 = ffn(x, identity=torch.zeros_like(x))
    torch.testing.assert_close(y3.float(), (y2.float() - x.float()), rtol=2e-3, atol=6e-3)
    # short inputs (the decoder's 900 queries) stay on the two-GEMM path: one fused block walks the whole hidden dim
    before = dict(_cabi.CALLS)
    with torch.no_grad():
        ys = ffn(x[:, :450])
    assert _cabi.CALLS["ffn_fused"] == before["ffn_fused"] and _cabi.CALLS["linear"] == before["linear"] + 2
    torch.testing.assert_close(ys.float(), y2[:, :450].float(), rtol=2e-3, atol=4e-3)


def test_ffn_layernorm_pos_epilogue_matches_three_kernels():
    """codetr_ffn_relu_ln_f16 == fused FFN -> codetr_layernorm_f16 -> fp16 add.  The epilogue normalises out of the
    accumulator layout: the same two-pass fp32 statistics as layernorm_kernel but summed in a different order (64 in-lane
    values, then the four lanes of a row), so a few outputs differ in the last fp16 bit; the `+ pos` output is exactly
    the kernel's own normalised output + pos."""
    from codetr import _cabi, hip_ops

    g = torch.Generator(device=DEV).manual_seed(3)
    M = 128 * 256 + 3333  # full round + 64-row tail launch
    x = torch.randn(M, 256, device=DEV, generator=g).half()
    pos = torch.randn(M, 256, device=DEV, generator=g).half()
    w1 = (torch.randn(2048, 256, device=DEV, generator=g) / 16).half()
    b1 = torch.randn(2048, device=DEV, generator=g).half()
    w2 = (torch.randn(256, 2048, device=DEV, generator=g) / 45).half()
    b2 = torch.randn(256, device=DEV, generator=g).half()
    gam = (1 + 0.1 * torch.randn(256, device=DEV, generator=g)).half()
    bet = (0.1 * torch.randn(256, device=DEV, generator=g)).half()
    y0 = hip_ops.ffn_fused(x, w1, b1, w2, b2)
    n0 = hip_ops.layer_norm(y0, gam, bet, 1e-5)
    before = _cabi.CALLS["layernorm"]
    n1 = hip_ops.ffn_fused(x, w1, b1, w2, b2, ln=(gam, bet, 1e-5))
    n2, q2 = hip_ops.ffn_fused(x, w1, b1, w2, b2, ln=(gam, bet, 1e-5), pos=pos)
    assert _cabi.CALLS["layernorm"] == before
    assert torch.equal(n1, n2)
    assert (n1 != n0).float().mean().item() < 0.02
    torch.testing.assert_close(n1.float(), n0.float(), rtol=0, atol=4e-3)   # 1 fp16 ulp at |value| < 4
    assert torch.equal(q2, n2 + pos)
    y3, q3 = hip_ops.ffn_fused(x, w1, b1, w2, b2, pos=pos)  # second output without the norm
    assert torch.equal(y3, y0) and torch.equal(q3, y0 + pos)
    # input LayerNorm folded in: == layer_norm -> fused FFN (+ LN + pos).  The statistics are summed in a different
    # lane order than layernorm_kernel's, so x1 may differ in the last fp16 bit on a few elements: 1-ulp tolerance on
    # the normalised output scale instead of bit equality
    gi = (1 + 0.1 * torch.randn(256, device=DEV, generator=g)).half()
    bi = (0.1 * torch.randn(256, device=DEV, generator=g)).half()
    t = (x * 3 + 1).half()
    x1 = hip_ops.layer_norm(t, gi, bi, 1e-5)
    r0, rq0 = hip_ops.ffn_fused(x1, w1, b1, w2, b2, ln=(gam, bet, 1e-5), pos=pos)
    before = _cabi.CALLS["layernorm"]
    r1, rq1 = hip_ops.ffn_fused(t, w1, b1, w2, b2, ln=(gam, bet, 1e-5), pos=pos, ln_in=(gi, bi, 1e-5))
    assert _cabi.CALLS["layernorm"] == before
    torch.testing.assert_close(r1.float(), r0.float(), rtol=0, atol=4e-3)
    torch.testing.assert_close(rq1.float(), rq0.float(), rtol=0, atol=8e-3)
    assert (r1 != r0).float().mean() < 0.02   # the vast majority of elements are bit-identical
    r2 = hip_ops.ffn_fused(t, w1, b1, w2, b2, ln_in=(gi, bi, 1e-5))    # input norm only
    torch.testing.assert_close(r2.float(), hip_ops.ffn_fused(x1, w1, b1, w2, b2).float(), rtol=0, atol=2e-2)


def test_encoder_layers_chain_through_the_fused_epilogue():
    """A post-norm (self_attn, norm, ffn, norm) encoder: LN2 and the next layer's `+ query_pos` come out of the FFN
    kernel (no separate layer-norm / add launches for them) and the result equals the unfused walk."""
    from codetr import _cabi, hip_ops
    from codetr.transformer import DetrTransformerEncoder

    torch.manual_seed(0)
    cfg = dict(type="BaseTransformerLayer",
               attn_cfgs=dict(type="MultiScaleDeformableAttention", embed_dims=256, num_levels=2, dropout=0.0),
               feedforward_channels=2048, ffn_dropout=0.0, operation_order=("self_attn", "norm", "ffn", "norm"))
    enc = DetrTransformerEncoder(transformerlayers=cfg, num_layers=3).to(DEV).half().eval()
    shapes = [(160, 160), (40, 40)]
    S = sum(h * w for h, w in shapes)
    assert S >= hip_ops.FFN_FUSED_MIN_ROWS
    g = torch.Generator(device=DEV).manual_seed(1)
    q = torch.randn(1, S, 256, device=DEV, generator=g).half()
    pos = torch.randn(1, S, 256, device=DEV, generator=g).half()
    ref = torch.rand(1, S, 2, 2, device=DEV, generator=g).half()
    ss = torch.tensor(shapes, device=DEV)
    ls = torch.tensor([0, shapes[0][0] * shapes[0][1]], device=DEV)
    mask = torch.zeros(1, S, dtype=torch.bool, device=DEV)
    kw = dict(reference_points=ref, spatial_shapes=ss, level_start_index=ls)
    before = dict(_cabi.CALLS)
    with torch.no_grad():
        out = enc.forward_bf(q, pos, mask, **kw)
    assert _cabi.CALLS["ffn_fused"] - before["ffn_fused"] == 3
    assert _cabi.CALLS["layernorm"] - before["layernorm"] == 0      # both norms of every layer ride in the FFN kernel
    saved = hip_ops.FFN_FUSED_MIN_ROWS
    try:
        hip_ops.FFN_FUSED_MIN_ROWS = 1 << 60                      # two-GEMM FFN, separate norms and adds
        with torch.no_grad():
            out0 = enc.forward_bf(q, pos, mask, **kw)
    finally:
        hip_ops.FFN_FUSED_MIN_ROWS = saved
    torch.testing.assert_close(out.float(), out0.float(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("M,hidden", [(129, 2048), (5000, 512), (30785, 2048)])
def test_ffn_fused_bf16_vs_fp32(M, hidden):
    """the bf16 instantiation (codetr_ffn_relu_ln2_bf16): hidden activation rounded to bf16 like the two-GEMM path"""
    from codetr import _cabi, hip_ops

    g = torch.Generator(device=DEV).manual_seed(M + hidden)
    bf = torch.bfloat16
    x = torch.randn(M, 256, device=DEV, generator=g).to(bf)
    w1 = (torch.randn(hidden, 256, device=DEV, generator=g) / 16).to(bf)
    b1 = (torch.randn(hidden, device=DEV, generator=g) * 0.5).to(bf)
    w2 = (torch.randn(256, hidden, device=DEV, generator=g) / hidden ** 0.5).to(bf)
    b2 = (torch.randn(256, device=DEV, generator=g) * 0.5).to(bf)
    before = _cabi.CALLS["ffn_fused"]
    y = hip_ops.ffn_fused(x, w1, b1, w2, b2)
    torch.cuda.synchronize()
    assert _cabi.CALLS["ffn_fused"] == before + 1 and y.dtype == bf
    h = torch.relu(x.float() @ w1.float().t() + b1.float()).to(bf).float()
    ref = (h @ w2.float().t() + b2.float()).to(bf).float() + x.float()
    torch.testing.assert_close(y.float(), ref, rtol=2e-2, atol=3e-2)   # bf16: 8 significant bits


def test_ffn_bf16_layernorm_pos_epilogue_matches_three_kernels():
    """bf16: fused (input LN, FFN, LN, + pos) against layer_norm -> fused FFN -> layer_norm -> add"""
    from codetr import hip_ops

    g = torch.Generator(device=DEV).manual_seed(5)
    bf = torch.bfloat16
    M = 128 * 64 + 77
    mk = lambda *s, sc=1.0: (torch.randn(*s, device=DEV, generator=g) * sc).to(bf)  # noqa: E731
    x, pos = mk(M, 256), mk(M, 256)
    w1, b1, w2, b2 = mk(2048, 256, sc=1 / 16), mk(2048), mk(256, 2048, sc=1 / 45), mk(256)
    gam, bet = (1 + mk(256, sc=0.1).float()).to(bf), mk(256, sc=0.1)
    y0 = hip_ops.ffn_fused(x, w1, b1, w2, b2)
    n0 = hip_ops.layer_norm(y0, gam, bet, 1e-5)
    n1, q1 = hip_ops.ffn_fused(x, w1, b1, w2, b2, ln=(gam, bet, 1e-5), pos=pos)
    assert (n1 != n0).float().mean().item() < 0.02 and torch.equal(q1, n1 + pos)   # (summation order: see the f16 test)
    torch.testing.assert_close(n1.float(), n0.float(), rtol=0, atol=3.2e-2)         # 1 bf16 ulp at |value| < 4
    x1 = hip_ops.layer_norm(x, gam, bet, 1e-5)
    r0 = hip_ops.ffn_fused(x1, w1, b1, w2, b2, ln=(gam, bet, 1e-5))
    r1 = hip_ops.ffn_fused(x, w1, b1, w2, b2, ln=(gam, bet, 1e-5), ln_in=(gam, bet, 1e-5))
    torch.testing.assert_close(r1.float(), r0.float(), rtol=0, atol=6e-2)
    assert (r1 != r0).float().mean() < 0.05


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,with_ln_in,with_pos", [(128 * 256 + 3333, True, True), (30785, True, False), (128 * 3 + 5, False, False)])
def test_ffn_with_output_projection_folded_in(M, with_ln_in, with_pos, dtype):
    """codetr_ffn_oproj_relu_ln2_*: x0 = identity + E(attn Wo^T + bo); x1 = LN_in(x0); y = LN(x1 + ffn(x1)) (+ pos) in ONE
    launch == codetr_linear_* with the residual epilogue, then the fused FFN kernel with ln_in.  The out-projection
    accumulates in a different order than the GEMM kernel and the norm statistics in a different lane order, so a few x1
    values differ in their last bit: 1 ulp of the normalised output scale, the vast majority bit-identical; and against the
    fp32 composition of the same operands."""
    from codetr import _cabi, hip_ops

    g = torch.Generator(device=DEV).manual_seed(M)
    r = lambda *s, k=1.0: (torch.randn(*s, device=DEV, generator=g) * k).to(dtype)   # noqa: E731
    attn, ident, pos = r(M, 256), r(M, 256, k=2.0), r(M, 256)
    wo, bo = r(256, 256, k=1 / 16), r(256, k=0.5)
    w1, b1 = r(2048, 256, k=1 / 16), r(2048)
    w2, b2 = r(256, 2048, k=1 / 45), r(256)
    gam, bet = (1 + 0.1 * torch.randn(256, device=DEV, generator=g)).to(dtype), r(256, k=0.1)
    gi, bi = (1 + 0.1 * torch.randn(256, device=DEV, generator=g)).to(dtype), r(256, k=0.1)
    ln, ln_in = (gam, bet, 1e-5), ((gi, bi, 1e-5) if with_ln_in else None)
    with torch.no_grad():
        x0 = hip_ops.linear(attn, wo, bo, residual=ident)
        ref = hip_ops.ffn_fused(x0, w1, b1, w2, b2, ln=ln, pos=pos if with_pos else None, ln_in=ln_in)
        before = dict(_cabi.CALLS)
        got = hip_ops.ffn_oproj_fused(attn, wo, bo, ident, w1, b1, w2, b2, ln, pos=pos if with_pos else None, ln_in=ln_in)
        torch.cuda.synchronize()
        assert _cabi.CALLS["ffn_oproj_fused"] == before["ffn_oproj_fused"] + 1
        assert _cabi.CALLS["linear"] == before["linear"] and _cabi.CALLS["layernorm"] == before["layernorm"]
    if not with_pos:
        ref, got = (ref,), (got,)
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    for a, b, scale in zip(got, ref, (4.0, 8.0)):
        assert a.shape == b.shape and a.dtype == dtype
        err = (a.float() - b.float()).abs()
        assert float(err.max()) <= 4 * ulp * scale, float(err.max())
        assert float((a != b).float().mean()) < (0.03 if dtype == torch.float16 else 0.06)
    if with_pos:
        assert torch.equal(got[1], got[0] + pos)
    # fp32 composition of the same operands (roundings at the same places as the kernels': E after the out-projection,
    # after the residual, after the norm, after the hidden activation, after the second product, after the last residual)
    E = lambda t: t.to(dtype).float()   # noqa: E731
    f0 = E(E(attn.float() @ wo.float().t() + bo.float()) + ident.float())
    f1 = E(torch.nn.functional.layer_norm(f0, (256,), gi.float(), bi.float(), 1e-5)) if with_ln_in else f0
    h = E(torch.relu(f1 @ w1.float().t() + b1.float()))
    f2 = E(E(h @ w2.float().t() + b2.float()) + f1)
    fy = torch.nn.functional.layer_norm(f2, (256,), gam.float(), bet.float(), 1e-5)
    err = (got[0].float() - fy).abs()
    # a 1-ulp flip of x1 moves the normalised output by a few ulp on the rows it touches: bound the mean tightly, the max loosely
    assert float(err.mean()) < ulp * 1.0 and float(err.max()) < 24 * ulp * 4.0, (float(err.mean()), float(err.max()))


def test_encoder_layer_defers_the_output_projection_into_the_ffn_launch():
    """DetrTransformerEncoder on the packed MSDA path: per layer ONE projection launch, the MSDA kernel, ONE FFN launch
    (output_proj, norm1, FFN, norm2, + query_pos inside) -- and the same result as with the switch off."""
    from codetr import _cabi, hip_ops
    from codetr.transformer import DetrTransformerEncoder

    torch.manual_seed(0)
    cfg = dict(type="BaseTransformerLayer",
               attn_cfgs=dict(type="MultiScaleDeformableAttention", embed_dims=256, num_levels=5, dropout=0.0),
               feedforward_channels=2048, ffn_dropout=0.0, operation_order=("self_attn", "norm", "ffn", "norm"))
    enc = DetrTransformerEncoder(transformerlayers=cfg, num_layers=2).to(DEV).half().eval()
    shapes = [(160, 200), (80, 100), (40, 50), (20, 25), (10, 13)]
    S = sum(h * w for h, w in shapes)
    g = torch.Generator(device=DEV).manual_seed(1)
    q = torch.randn(1, S, 256, device=DEV, generator=g).half()
    pos = torch.randn(1, S, 256, device=DEV, generator=g).half()
    from codetr.transformer import _shape_tensors

    ss, ls = _shape_tensors(shapes, torch.device(DEV))
    mask = torch.zeros(1, S, dtype=torch.bool, device=DEV)
    vr = torch.ones(1, 5, 2, device=DEV, dtype=torch.float16)
    _, ref, _, _ = hip_ops.encoder_geometry(vr, mask, shapes)
    # fp32 reference points from the valid pixel counts (the packed kernel's contract): an unpadded image
    ref._codetr_valid_counts = torch.tensor([[[w, h] for h, w in shapes]], dtype=torch.float32, device=DEV)
    kw = dict(reference_points=ref, spatial_shapes=ss, level_start_index=ls)
    before = dict(_cabi.CALLS)
    with torch.no_grad():
        out = enc.forward_bf(q, pos, mask, **kw)
    d = {k: _cabi.CALLS[k] - before[k] for k in ("ffn_oproj_fused", "encoder_projections", "msda_encoder_packed", "layernorm")}
    assert d == {"ffn_oproj_fused": 2, "encoder_projections": 2, "msda_encoder_packed": 2, "layernorm": 0}, d
    hip_ops.FFN_OPROJ = False
    try:
        with torch.no_grad():
            out0 = enc.forward_bf(q, pos, mask, **kw)
    finally:
        hip_ops.FFN_OPROJ = True
    torch.testing.assert_close(out.float(), out0.float(), rtol=0, atol=1.6e-2)
    assert float((out.float() - out0.float()).abs().mean()) < 1e-3


# ----------------------------------------------------------------------------------------------------------------------
# float64 interval bounds, exact routing, tails (tests/ffn_bounds.py; proved on the CPU by tests/test_ffn_bounds_cpu.py).
# Every case runs through the _cabi entries that take the output tensors, which carry GUARD rows of a bit pattern behind
# row M; the row counts come from the device's CU count.
import ffn_bounds as fb  # noqa: E402

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
GUARD, PATTERN = 256, 0x5a5a


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _guarded(M, dtype):
    return torch.full((M + GUARD, 256), PATTERN, dtype=torch.int16, device=DEV).view(dtype)


def _run(inp):
    """-> (Y, Y2 | None), [M, 256] each; asserts that the guard rows kept their bits"""
    from codetr import _cabi

    dt, M = inp["dtype"], inp["x"].shape[0]
    w2p = _cabi.ffn_pack_w2(inp["w2"].contiguous())
    y = _guarded(M, dt)
    y2 = _guarded(M, dt) if "pos" in inp else None
    args = dict(ln=inp.get("ln"), ln_in=inp.get("ln_in"), pos2d=inp.get("pos"), out_plus_pos2d=y2)
    if "wo" in inp:
        idx = torch.tensor(_cabi.ffn_oproj_w1_index(256), device=DEV)
        _cabi.ffn_oproj_fused(inp["x"], inp["wo"], inp["bo"], inp["ident"], inp["w1"][:, idx].contiguous(), inp["b1"], w2p,
                              inp["b2"], y, **args)
    else:
        _cabi.ffn_fused(inp["x"], inp["w1"], inp["b1"], w2p, inp["b2"], y, **args)
    torch.cuda.synchronize()
    for t in (y, y2):
        assert t is None or bool((t[M:].view(torch.int16) == PATTERN).all()), "rows behind M were written"
    return y[:M], (y2[:M] if y2 is not None else None)


def _bits(t):
    return t.contiguous().view(torch.int16)


@DTYPES
@pytest.mark.parametrize("name", [n for n in fb.FFN_CASE_NAMES if not n.startswith(("exact", "routing"))])
def test_ffn_within_the_float64_bound_and_share(name, dtype):
    """every element within the derived bound of the float64 reference, and no more elements off the exact value than 4 x
    the emulation's share on the same inputs"""
    cus = _cus()
    case = fb.ffn_cases(cus)[name]
    for M in case.Ms:
        plan = fb.ffn_plan(M, case.hidden, cus)
        assert tuple(l.form for l in plan.launches) == case.forms and plan.walk == case.walk
    res = fb.measure(case, dtype, _run, DEV, cus)
    print(f"ffn {name} {dtype}: err/bound {res.ratio:.3f} (emulated {res.emu_ratio:.3f})  share {res.share:.5f} "
          f"(emulated {res.emu_share:.5f}, cap {fb.share_cap(res):.5f})")
    assert res.ratio <= 1.0
    assert res.share <= fb.share_cap(res)


@DTYPES
@pytest.mark.parametrize("name", [n for n in fb.FFN_CASE_NAMES if n.startswith(("exact", "routing"))])
def test_ffn_exact_small_integers_pin_the_lane_maps_the_packs_and_the_row_offset(name, dtype):
    """bit equality with float64: sparse +-1 weights on small integers, and one-hot W1 / W2 (/ Wo) on one integer per (row of a
    16-row tile, column) -- the W2 k-slot pack, the oproj W1 column exchange, the LDS swizzles, the epilogue's half swap, the
    second launch's row offset"""
    from codetr import _cabi

    cus = _cus()
    case = fb.ffn_cases(cus)[name]
    assert torch.equal(torch.tensor(_cabi.ffn_oproj_w1_index(256)), fb.oproj_w1_index())
    for M in case.Ms:
        inp = fb.to_device(fb.build(case, M, dtype), DEV)
        assert torch.equal(_cabi.ffn_pack_w2(inp["w2"].contiguous()), inp["w2"][:, fb.pack_w2_index(case.hidden).to(DEV)])
        ex = fb.exact_ffn(inp)
        y, y2 = _run(inp)
        for got, want, what in ((y, ex.out, "Y"), (y2, ex.out2, "Y2")):
            bad = (got.double() != want).nonzero()
            assert bad.numel() == 0, (what, M, bad[:4].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


@DTYPES
@pytest.mark.parametrize("M", [200, None], ids=["64row", "128row"])
def test_ffn_distinct_norms_return_their_own_beta_on_constant_rows(M, dtype):
    """ln_in_eps = 1e-3, ln_eps = 1e-5 on rows of variance 1e-4 .. 1e-3, different gamma / beta: with W2 = b2 = 0 the kernel's
    output IS x1, whose constant row 0 is beta_in bit for bit; with the output norm alone, row 1 (x = 0, h = 0, t = b2) is beta"""
    cus = _cus()
    M = M or fb.ragged_M(cus)
    inp = fb.to_device(fb.ffn_distinct(M, 256, dtype, "ln_in"), DEV)
    inp["w2"], inp["b2"] = torch.zeros_like(inp["w2"]), torch.zeros_like(inp["b2"])
    ex = fb.exact_ffn(inp)
    x1, _ = _run(inp)
    assert torch.equal(_bits(x1[0]), _bits(inp["ln_in"][1]))
    assert fb.ratio(x1, ex.out, fb.bound(ex).out) <= 1.0
    inp = fb.to_device(fb.ffn_distinct(M, 256, dtype, "ln"), DEV)
    ex = fb.exact_ffn(inp)
    y, _ = _run(inp)
    assert torch.equal(_bits(y[1]), _bits(inp["ln"][1]))
    assert fb.ratio(y, ex.out, fb.bound(ex).out) <= 1.0


@DTYPES
@pytest.mark.parametrize("form", ["plain_pos", "full", "oproj"])
def test_ffn_guard_rows_keep_their_bits(form, dtype):
    """256 rows of a bit pattern behind row M of Y and Y2, at the tail, the ragged and the split row counts (`_run` asserts it
    on every call of this module; here by name)"""
    cus = _cus()
    for M in fb.TAIL_M + (fb.ragged_M(cus), fb.split_M(cus)):
        y, y2 = _run(fb.to_device(fb.ffn_random(M, 128, dtype, form), DEV))
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(y2).all())


@DTYPES
@pytest.mark.parametrize("form", ["plain_pos", "full", "oproj"])
def test_ffn_rows_are_isolated_from_a_non_finite_row(form, dtype):
    """one row set to +inf, NaN or 65504 -- row M - 1 of a ragged tile (the row every clamped lane reads) and a row in the
    middle of a 16-row tile: every other row has the bits of the run with that row zeroed (the epilogues move data between
    lanes: __shfl_xor 16, ds_bpermute)"""
    cus = _cus()
    for M in (200, fb.ragged_M(cus)):
        base = fb.to_device(fb.ffn_random(M, 128, dtype, form), DEV)
        for row in (M - 1, 16 * ((M - 1) // 32) + 7):
            keep = torch.arange(M, device=DEV) != row
            zeroed = dict(base, x=base["x"].clone())
            zeroed["x"][row] = 0
            want = _run(zeroed)
            for value in (float("inf"), float("nan"), 65504.0):
                bad = dict(base, x=base["x"].clone())
                bad["x"][row] = value
                for got, ref in zip(_run(bad), want):
                    assert torch.equal(_bits(got[keep]), _bits(ref[keep])), (M, row, value)


@DTYPES
@pytest.mark.parametrize("form", ["full", "oproj"])
def test_ffn_one_row_one_result_in_the_64_row_and_the_128_row_form(form, dtype):
    """the same rows give the same bits in a small call (the 64-row form) and inside a large one (the 128-row form), 37 rows
    further down"""
    cus = _cus()
    M = fb.ragged_M(cus)
    big = fb.to_device(fb.ffn_random(M, 256, dtype, form), DEV)
    assert [l.form for l in fb.ffn_plan(M, 256, cus).launches] == [128] and [l.form for l in fb.ffn_plan(150, 256, cus).launches] == [64]
    small = {k: (v[37:187].contiguous() if torch.is_tensor(v) and v.shape[0] == M and k in ("x", "ident", "pos") else v)
             for k, v in big.items()}
    for a, b in zip(_run(small), _run(big)):
        assert torch.equal(_bits(a), _bits(b[37:187]))
