"""Dense multi-head attention kernel (csrc/mha_attention.hip, codetr_mha_attention_*) against the float64 formula
softmax(q k^T / sqrt(32)) v -- the core of nn.MultiheadAttention in the decoder's self-attention (reference
transformer_mmcv.py:394-428) -- within the bound derived from where the kernel rounds (tests/attention_bounds.py, proved on
the CPU by tests/test_attention_bounds_cpu.py).

Random cases (`bound`): the decoder shape (900 queries, 8 heads), key counts around the 128-key chunk and 32-row padding
boundaries, strided q / k views of a fused projection, large logits, bf16.  Each also asserts that the bound is nowhere above
the rtol / atol it replaced.

Structured cases (`structured_tol`: the probabilities are exactly 0, 1 or all equal):
  uniform   q = 0: the mean of v over exactly the Nk real keys, the last key's row is 32 (key tail, pad keys in the sum)
  routing   +-9 binary codes: row i must be v[target(i)] (V rows, key order, both directions of the online-softmax rescale)
  graded    two score levels whose lower probability sits just below a storage step (`bound`): rounded, not truncated

Largest err / bound over the random cases:
  measured on MI355X   fp16 0.53   bf16 0.31
  emulated on the CPU  fp16 0.53   bf16 0.31"""
import os
import sys

import pytest
import torch

import attention_bounds as ab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT = {torch.float16: "f16", torch.bfloat16: "bf16"}
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def _ref(q, k, v, H):
    B, Nq, C = q.shape
    sp = lambda t: t.float().reshape(B, -1, H, 32).transpose(1, 2)  # noqa: E731
    a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / 32 ** 0.5, -1)
    return (a @ sp(v)).transpose(1, 2).reshape(B, Nq, C)


def _within_bound(out, q, k, v, H, rtol, atol, what):
    """|out - float64| <= bound elementwise, and the bound nowhere above the tolerance it replaced"""
    ex = ab.exact_mha(q, k, v, H)
    b = ab.bound(ex).total
    r = ab.ratio(out, ex, b)
    print(f"mha {what}: err/bound {r:.3f}")
    assert (b <= rtol * ex.out.abs() + atol).all()
    assert r < 1, what


def _within_structured(out, ex, what, tol=None):
    r = ab.ratio(out, ex, ab.structured_tol(ex) if tol is None else tol)
    print(f"mha {what}: err/tol {r:.3f}")
    assert r < 1, what


@pytest.mark.parametrize("B,N,H", ab.DENSE_RANDOM)
def test_matches_fp32_softmax_attention(B, N, H):
    from codetr import _cabi, hip_ops

    q, k, v = ab.dense_random(B, N, N, H, torch.float16, N + H, DEV)
    before = _cabi.CALLS["mha_attention"]
    out = hip_ops.mha_self_attention(q, k, v, H)
    torch.cuda.synchronize()
    assert _cabi.CALLS["mha_attention"] == before + 1
    _within_bound(out, q, k, v, H, 5e-3, 3e-3, f"f16 B{B} N{N} H{H}")


def test_strided_views_of_a_fused_projection_and_cross_lengths():
    """q | k as column halves of one [B, N, 2C] tensor (what MultiheadAttention.forward_bf passes); Nq != Nk"""
    from codetr import _cabi

    H, C = 8, 256
    qk, v, q2 = ab.dense_strided(DEV)
    q, k = qk[..., :C], qk[..., C:]
    assert _cabi.mha_attention_supported(q, k, v, H)
    out = torch.empty(2, 300, C, dtype=torch.float16, device=DEV)
    _cabi.mha_attention(q, k, v, H, out)
    _within_bound(out, q, k, v, H, 5e-3, 3e-3, "f16 strided 300x300")
    out2 = torch.empty(2, 70, C, dtype=torch.float16, device=DEV)          # fewer queries than keys
    _cabi.mha_attention(q2, k, v, H, out2)
    _within_bound(out2, q2, k, v, H, 5e-3, 3e-3, "f16 strided 70x300")


def test_large_logits_stay_finite():
    from codetr import hip_ops

    # logits of several hundred: the running max must keep exp2 in range
    q, k, v = ab.dense_random(1, 400, 400, 2, torch.float16, 2, DEV, q_scale=30.0)
    out = hip_ops.mha_self_attention(q, k, v, 2)
    assert torch.isfinite(out).all()
    _within_bound(out, q, k, v, 2, 5e-3, 5e-3, "f16 q x 30")


def test_bf16_and_fallback():
    from codetr import _cabi, hip_ops

    q, k, v = ab.dense_random(2, 333, 333, 4, torch.bfloat16, 3, DEV)
    out = hip_ops.mha_self_attention(q, k, v, 4)
    _within_bound(out, q, k, v, 4, 2e-2, 2e-2, "bf16 B2 N333 H4")
    before = _cabi.CALLS["mha_attention"]
    g = torch.Generator(device=DEV).manual_seed(3)
    q, k, v = (torch.randn(1, 1500, 64, device=DEV, generator=g).half() for _ in range(3))   # > 1024 keys: library path
    out = hip_ops.mha_self_attention(q, k, v, 2)
    assert _cabi.CALLS["mha_attention"] == before
    torch.testing.assert_close(out.float(), _ref(q, k, v, 2), rtol=5e-3, atol=3e-3)


def _run(q, k, v, H=3):
    from codetr import _cabi

    assert _cabi.mha_attention_supported(q, k, v, H)
    out = torch.empty(q.shape, dtype=q.dtype, device=DEV)
    _cabi.mha_attention(q, k, v, H, out)
    torch.cuda.synchronize()
    return out


@DTYPES
@pytest.mark.parametrize("Nk", ab.DENSE_UNIFORM_NK)
def test_uniform_scores_give_the_mean_over_the_real_keys(Nk, dtype):
    """pad keys in the row sum scale the result by Nk / NP; a dropped tail key removes the 32"""
    q, k, v = ab.dense_uniform(Nk, dtype, DEV)
    _within_structured(_run(q, k, v), ab.exact_mha(q, k, v, 3), f"{DT[dtype]} uniform Nk{Nk}")


@DTYPES
@pytest.mark.parametrize("Nq,Nk", ab.DENSE_ROUTING)
def test_routing_returns_the_target_row(Nq, Nk, dtype):
    q, k, v = ab.dense_routing(Nq, Nk, dtype, DEV)
    ex = ab.exact_mha(q, k, v, 3)
    t = ab.routing_target(Nq, Nk, 2, 3).to(DEV)
    want = torch.gather(v.view(2, Nk, 3, 32).transpose(1, 2), 2, t[..., None].expand(-1, -1, -1, 32))
    assert (ex.out - want.transpose(1, 2).reshape(2, Nq, 96).double()).abs().max() < 1e-9      # the float64 value IS v[target]
    _within_structured(_run(q, k, v), ex, f"{DT[dtype]} routing {Nq}x{Nk}")


@DTYPES
def test_routing_through_the_column_halves_of_a_fused_projection(dtype):
    """the same construction at the decoder's 900 x 900, q | k being strided views of one [B, N, 2C] tensor"""
    q, k, v = ab.dense_routing(*ab.DENSE_ROUTING_FUSED, dtype, DEV)
    qk = torch.cat((q, k), -1)
    q, k = qk[..., :96], qk[..., 96:]
    assert not q.is_contiguous() and not k.is_contiguous()
    _within_structured(_run(q, k, v), ab.exact_mha(q, k, v, 3), f"{DT[dtype]} routing fused 900x900")


@DTYPES
@pytest.mark.parametrize("Nq,Nk", ab.DENSE_GRADED)
def test_graded_probabilities_are_rounded_not_truncated(Nq, Nk, dtype):
    q, k, v = ab.dense_graded(Nq, Nk, dtype, DEV)
    ex = ab.exact_mha(q, k, v, 3)
    _within_structured(_run(q, k, v), ex, f"{DT[dtype]} graded {Nq}x{Nk}", tol=ab.bound(ex).total)
