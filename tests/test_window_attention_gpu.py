"""The fused Swin window-attention kernel (csrc/window_attention.hip, codetr_window_attention_*) against the reference's
tensor program for the same step -- pad (zeros -> qkv bias), roll, window partition, q*scale @ k^T + relative-position bias
+ (-100) shift mask, softmax, @ v, window reverse, roll back, crop (reference codetr/swin.py:191-252, 92-112) -- evaluated
in float64 on the 16-bit inputs (tests/attention_bounds.py: exact_window), within the bound derived from where the kernel
rounds (`bound`, proved on the CPU by tests/test_attention_bounds_cpu.py).  Each random case also asserts that the bound is
nowhere above the rtol / atol it replaced (fp16 5e-3 / 3e-3, bf16 2e-2 / 2e-2).

Structured cases (`structured_tol`: the probabilities are exactly 0, 1 or all equal):
  uniform regions   q = 0, zero table: the mean of v over the query's own shift-mask region, pad tokens (v = 16) included
  routing           q = 0, one table offset per head at 48: the target token's v (a pad token's: the bias) where the target is
                    in the window and region, the region mean where it is masked; both bias layouts
  graded            one offset at 0, the rest at -gap with exp(-gap) just below a storage step (`bound`): rounded, not truncated

Largest err / bound over the random cases:
  measured on MI355X   fp16 0.69   bf16 0.66
  emulated on the CPU  fp16 0.69   bf16 0.66"""
import pytest
import torch

import attention_bounds as ab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DT = {torch.float16: "f16", torch.bfloat16: "bf16"}
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def _rel_bias(table, nH, ws):
    """[nH, N, N] as the model gathers it from a table that is already in the storage type"""
    from codetr.swin import WindowMSA

    m = WindowMSA(nH * 32, nH, (ws, ws)).to(DEV).to(table.dtype)
    with torch.no_grad():
        m.relative_position_bias_table.copy_(table)
    rb = m.relative_position_bias()
    assert torch.equal(rb, ab.gather_bias(table, ws))
    return rb


def _run(x, H, W, nH, ws, shift):
    from codetr import hip_ops

    qkv, qkv_bias, table = x
    out = hip_ops.swin_window_attention(qkv, qkv_bias, _rel_bias(table, nH, ws), (H, W), nH, ws, shift)
    torch.cuda.synchronize()
    assert out.dtype == qkv.dtype
    return out


def _case(B, H, W, nH, ws, shift, seed=0, bias_scale=1.0, dtype=torch.float16):
    x = ab.window_random(B, H, W, nH, ws, shift, seed, bias_scale, dtype, DEV)
    out = _run(x, H, W, nH, ws, shift)
    ex = ab.exact_window(*x, H, W, nH, ws, shift)
    b = ab.bound(ex).total
    r = ab.ratio(out, ex, b)
    print(f"window {DT[dtype]} B{B} {H}x{W} nH{nH} ws{ws} s{shift} bias x{bias_scale:g}: "
          f"err/bound {r:.3f}")
    rtol, atol = ab.window_legacy_tol(dtype)
    assert (b <= rtol * ex.out.abs() + atol).all()       # nowhere weaker than the tolerance this bound replaced
    assert r < 1


def _structured(x, geo, what, full_bound=False):
    ex = ab.exact_window(*x, *geo)
    r = ab.ratio(_run(x, *geo), ex, ab.bound(ex).total if full_bound else ab.structured_tol(ex))
    print(f"window {DT[x[0].dtype]} {what}: err/tol {r:.3f}")
    assert r < 1, what


@DTYPES
@pytest.mark.parametrize("ws,shift,H,W", ab.WINDOW_STRUCTURED)
def test_uniform_scores_give_the_region_mean(ws, shift, H, W, dtype):
    _structured(ab.window_uniform(ws, shift, H, W, dtype, DEV), (H, W, 3, ws, shift), f"uniform ws{ws} s{shift} {H}x{W}")


@DTYPES
@pytest.mark.parametrize("lane", [True, False], ids=["lane", "table"])
@pytest.mark.parametrize("ws,shift,H,W", ab.WINDOW_STRUCTURED)
def test_table_routes_to_the_target_token(ws, shift, H, W, lane, dtype):
    """pins the lane-order permutation of the bias by value, not only against the other layout"""
    from codetr import hip_ops

    hip_ops.WINDOW_BIAS_LANE = lane
    try:
        _structured(ab.window_routing(ws, shift, H, W, dtype, DEV), (H, W, 3, ws, shift),
                    f"routing ws{ws} s{shift} {H}x{W} {'lane' if lane else 'table'}")
    finally:
        hip_ops.WINDOW_BIAS_LANE = True


@DTYPES
@pytest.mark.parametrize("ws,shift,H,W", ab.WINDOW_GRADED)
def test_graded_probabilities_are_rounded_not_truncated(ws, shift, H, W, dtype):
    _structured(ab.window_graded(ws, shift, H, W, dtype, DEV), (H, W, 3, ws, shift), f"graded ws{ws} s{shift} {H}x{W}",
                full_bound=True)


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("B,H,W,nH", [
    (1, 12, 12, 1),      # exactly one window
    (2, 24, 36, 2),      # no padding
    (1, 20, 31, 6),      # pads both ways (24 x 36), stage-0 head count
    (3, 13, 12, 3),      # pad rows only, odd head count (wave tail)
    (1, 40, 60, 4),      # 1920x1280 stage-3 map: pads H 40 -> 48
])
def test_window12(B, H, W, nH, shift):
    _case(B, H, W, nH, 12, shift, seed=H + W + shift)


@pytest.mark.parametrize("ws,shift,H,W", [(7, 0, 14, 14), (7, 3, 16, 20), (8, 4, 17, 9), (4, 2, 11, 15), (4, 0, 8, 8)])
def test_other_window_sizes(ws, shift, H, W):
    _case(2, H, W, 2, ws, shift, seed=ws)


@pytest.mark.parametrize("ws,shift,B,H,W,nH", [(12, 0, 2, 24, 36, 2), (12, 6, 1, 20, 31, 6), (7, 3, 2, 16, 20, 2),
                                               (12, 6, 1, 40, 60, 4)])
def test_bf16(ws, shift, B, H, W, nH):
    """the bf16 instantiation (codetr_window_attention_bf16) against the same float64 restatement"""
    _case(B, H, W, nH, ws, shift, seed=ws + H, dtype=torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ws,shift,H,W,nH", [(12, 0, 24, 36, 2), (12, 6, 20, 31, 6), (8, 4, 17, 9, 2), (4, 2, 11, 15, 3), (4, 0, 8, 8, 2)])
def test_lane_order_bias_is_bit_identical(ws, shift, H, W, nH, dtype):
    """bias_layout 1 of codetr_window_attention_ex (the table permuted into the kernel's lane order, what the model
    launches) against layout 0 (the reference's [nH, N, N]): same values through different loads -> the same bits; and
    the index the permutation comes from"""
    from codetr import _cabi, hip_ops
    from codetr.swin import WindowMSA

    idx = _cabi.window_attention_bias_index(ws)
    NT = ws * ws // 16
    assert idx == [16 * kt + 4 * g + r for g in range(4) for kt in range(NT) for r in range(4)]
    assert _cabi.window_attention_bias_index(7) is None
    C = nH * 32
    g = torch.Generator(device=DEV).manual_seed(ws + H)
    qkv = torch.randn(2, H * W, 3 * C, device=DEV, generator=g).to(dtype)
    qkv_bias = (0.5 * torch.randn(3 * C, device=DEV, generator=g)).to(dtype)
    m = WindowMSA(C, nH, (ws, ws)).to(DEV).to(dtype)
    with torch.no_grad():
        m.relative_position_bias_table.copy_(torch.randn(m.relative_position_bias_table.shape, device=DEV, generator=g))
    outs = []
    for lane in (True, False):
        hip_ops.WINDOW_BIAS_LANE = lane
        try:
            outs.append(hip_ops.swin_window_attention(qkv, qkv_bias, m.relative_position_bias(), (H, W), nH, ws, shift))
        finally:
            hip_ops.WINDOW_BIAS_LANE = True
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_large_logits_and_mask_dominance():
    """big relative-position biases: softmax must stay finite and the -100 mask must still win."""
    _case(1, 30, 30, 2, 12, 6, seed=9, bias_scale=8.0)


def test_swin_block_fused_matches_oracle():
    """ShiftWindowMSA through the fused path inside a 2-stage Swin (window 12, head_dim 32, padding at both
    stages) against the CPU oracle on the same weights."""
    import numpy as np

    import codetr_fp32 as M
    from codetr.swin import SwinTransformer
    from helpers_model import assert_close_lowp, seeded_params

    s = SwinTransformer(pretrain_img_size=64, embed_dims=64, depths=(2, 2), num_heads=(2, 4), window_size=12,
                        strides=(4, 2), out_indices=(0, 1), drop_path_rate=0.0, patch_norm=True)
    spec = [(k, tuple(v.shape)) for k, v in s.named_parameters()]
    sd = seeded_params(spec, 11, scale=1.5)
    s.load_state_dict(sd, strict=False)
    s = s.to(DEV).half().eval()
    img = torch.randn(2, 3, 100, 150, generator=torch.Generator().manual_seed(3))  # 25 x 38 tokens -> pads to 36 x 48
    from codetr import _cabi

    before = dict(_cabi.CALLS)
    with torch.no_grad():
        outs = s(img.to(DEV).half())
    assert _cabi.CALLS["window_attention"] - before["window_attention"] == 4  # every block took the fused kernel
    # qkv, proj, fc1, fc2 per block + 1 merge + the stem (patch gather + GEMM)
    assert _cabi.CALLS["linear"] - before["linear"] == 4 * 4 + 1 + 1
    assert _cabi.CALLS["patch_im2col"] - before["patch_im2col"] == 1
    assert _cabi.CALLS["layernorm"] > before["layernorm"]
    ref = M.swin_forward({"backbone." + k: v for k, v in sd.items()}, img, num_heads=(2, 4), window_size=12,
                         out_indices=(0, 1))
    for i in range(2):
        assert_close_lowp(outs[i].float().cpu().numpy(), ref[i].numpy(), 1e-2, 0.1, f"swin out {i}")
