"""The attention bound and the structured attention cases, proved on the CPU before a kernel is held to them
(tests/attention_bounds.py; the kernels run in tests/test_mha_attention_gpu.py and tests/test_window_attention_gpu.py).

(a) the emulation of each kernel's rounding points stays inside the tolerance of every case the GPU modules run, at the same
    shapes and values: `bound` for the random and graded cases, `structured_tol` for the uniform and routing cases;
(b) every mutant of the emulation leaves the tolerance in a structured case, for fp16 and for bf16 -- CATCH_* says which family
    must catch which mutant;
(c) on the unit-scale Gaussian cases the fp32 terms of the bound stay below u A / 4 elementwise: the bound is the storage
    roundings, and cannot be inflated through the fp32 terms unnoticed;
plus: no random case is held to less than the rtol / atol it was held to before, and the constructions are what they claim.

Run with -s to see the largest err / bound per case and the catching cases per mutant."""
import math

import pytest
import torch

import attention_bounds as ab

F16, BF16 = torch.float16, torch.bfloat16
DT = {F16: "f16", BF16: "bf16"}

CATCH_DENSE = {"drop_last_key": "uniform", "pads_counted": "uniform", "swap_v_rows": "routing", "truncate_p": "graded"}
CATCH_WINDOW = {"drop_last_key": "uniform", "pads_counted": "uniform", "swap_v_rows": "routing", "truncate_p": "graded",
                "wrong_region_one_key": "uniform", "pad_token_reads_zero": "uniform", "bias_row_shifted": "routing"}


def _dense_structured(dtype):
    """(family, name, (q, k, v), H)"""
    for Nk in ab.DENSE_UNIFORM_NK:
        yield "uniform", f"Nk{Nk}", ab.dense_uniform(Nk, dtype), 3
    for Nq, Nk in ab.DENSE_ROUTING + [ab.DENSE_ROUTING_FUSED]:
        yield "routing", f"{Nq}x{Nk}", ab.dense_routing(Nq, Nk, dtype), 3
    for Nq, Nk in ab.DENSE_GRADED:
        yield "graded", f"{Nq}x{Nk}", ab.dense_graded(Nq, Nk, dtype), 3


def _window_structured(dtype):
    """(family, name, (qkv, qkv_bias, table), (H, W, nH, ws, shift))"""
    for ws, shift, H, W in ab.WINDOW_STRUCTURED:
        yield "uniform", f"ws{ws} s{shift} {H}x{W}", ab.window_uniform(ws, shift, H, W, dtype), (H, W, 3, ws, shift)
        yield "routing", f"ws{ws} s{shift} {H}x{W}", ab.window_routing(ws, shift, H, W, dtype), (H, W, 3, ws, shift)
    for ws, shift, H, W in ab.WINDOW_GRADED:
        yield "graded", f"ws{ws} s{shift} {H}x{W}", ab.window_graded(ws, shift, H, W, dtype), (H, W, 3, ws, shift)


def _tol(family, ex):
    return ab.structured_tol(ex) if family in ("uniform", "routing") else ab.bound(ex).total


@pytest.fixture(scope="module")
def dense_exact():
    return {dt: [(fam, name, x, H, ab.exact_mha(*x, H)) for fam, name, x, H in _dense_structured(dt)] for dt in (F16, BF16)}


@pytest.fixture(scope="module")
def window_exact():
    return {dt: [(fam, name, x, geo, ab.exact_window(*x, *geo)) for fam, name, x, geo in _window_structured(dt)]
            for dt in (F16, BF16)}


# ------------------------------------------------------------------------------------------------------- (a), (c), part 4
def test_dense_random_cases_emulation_inside_bound_and_no_weaker_than_before():
    worst = {}
    for name, q, k, v, H, (rtol, atol), unit in ab.dense_random_inputs():
        ex = ab.exact_mha(q, k, v, H)
        b = ab.bound(ex)
        r = ab.ratio(ab.emulate_mha(q, k, v, H), ex, b.total)
        print(f"dense random {name}: emulated err/bound {r:.3f}")
        assert r < 1, name
        assert (b.total <= rtol * ex.out.abs() + atol).all(), name
        if unit:
            c = (b.fp32 / (ab.U[q.dtype] * ex.A)).max().item()
            print(f"    fp32 terms / (u A) {c:.4f}")
            assert c < 0.25, name
        worst[DT[q.dtype]] = max(worst.get(DT[q.dtype], 0), r)
    print("dense random, largest emulated err/bound:", worst)


def test_window_random_cases_emulation_inside_bound_and_no_weaker_than_before():
    worst = {}
    for B, H, W, nH, ws, shift, seed, bias_scale, dtype in ab.window_random_cases():
        name = f"{DT[dtype]} B{B} {H}x{W} nH{nH} ws{ws} s{shift} bias x{bias_scale:g}"
        x = ab.window_random(B, H, W, nH, ws, shift, seed, bias_scale, dtype)
        ex = ab.exact_window(*x, H, W, nH, ws, shift)
        b = ab.bound(ex)
        r = ab.ratio(ab.emulate_window(*x, H, W, nH, ws, shift), ex, b.total)
        print(f"window random {name}: emulated err/bound {r:.3f}")
        assert r < 1, name
        rtol, atol = ab.window_legacy_tol(dtype)
        assert (b.total <= rtol * ex.out.abs() + atol).all(), name
        if bias_scale == 1.0:
            c = (b.fp32 / (ab.U[dtype] * ex.A)).max().item()
            print(f"    fp32 terms / (u A) {c:.4f}")
            assert c < 0.25, name
        worst[DT[dtype]] = max(worst.get(DT[dtype], 0), r)
    print("window random, largest emulated err/bound:", worst)


def test_dense_structured_cases_emulation_inside_tolerance(dense_exact):
    for dt in (F16, BF16):
        for fam, name, x, H, ex in dense_exact[dt]:
            r = ab.ratio(ab.emulate_mha(*x, H), ex, _tol(fam, ex))
            print(f"dense {fam} {DT[dt]} {name}: emulated err/tol {r:.3f}")
            assert r < 1, (fam, name, dt)


def test_window_structured_cases_emulation_inside_tolerance(window_exact):
    for dt in (F16, BF16):
        for fam, name, x, geo, ex in window_exact[dt]:
            r = ab.ratio(ab.emulate_window(*x, *geo), ex, _tol(fam, ex))
            print(f"window {fam} {DT[dt]} {name}: emulated err/tol {r:.3f}")
            assert r < 1, (fam, name, dt)


# ------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("mutant", ab.DENSE_MUTANTS)
def test_dense_mutant_is_caught(mutant, dense_exact):
    for dt in (F16, BF16):
        caught = {}
        for fam, name, x, H, ex in dense_exact[dt]:
            r = ab.ratio(ab.emulate_mha(*x, H, mutant=mutant), ex, _tol(fam, ex))
            if r > 1:
                caught.setdefault(fam, []).append(f"{name} ({r:.3g}x)")
        print(f"dense {mutant} {DT[dt]}: caught by {caught}")
        assert CATCH_DENSE[mutant] in caught, (mutant, dt, caught)


@pytest.mark.parametrize("mutant", ab.WINDOW_MUTANTS)
def test_window_mutant_is_caught(mutant, window_exact):
    for dt in (F16, BF16):
        caught = {}
        for fam, name, x, geo, ex in window_exact[dt]:
            r = ab.ratio(ab.emulate_window(*x, *geo, mutant=mutant), ex, _tol(fam, ex))
            if r > 1:
                caught.setdefault(fam, []).append(f"{name} ({r:.3g}x)")
        print(f"window {mutant} {DT[dt]}: caught by {caught}")
        assert CATCH_WINDOW[mutant] in caught, (mutant, dt, caught)


# ------------------------------------------------------------------------------------------------------- the constructions
def test_uniform_and_routing_expectations_in_closed_form():
    """the float64 helpers give what the cases are built to give: the mean over the real keys, and v[target]"""
    for Nk in (1, 33, 897):
        q, k, v = ab.dense_uniform(Nk, F16)
        ex = ab.exact_mha(q, k, v, 3)
        assert torch.allclose(ex.out, v.double().mean(1, keepdim=True).expand_as(ex.out), rtol=0, atol=1e-12)
    for Nq, Nk in ab.DENSE_ROUTING:
        q, k, v = ab.dense_routing(Nq, Nk, BF16)
        ex = ab.exact_mha(q, k, v, 3)
        t = ab.routing_target(Nq, Nk, 2, 3)                                     # [B, H, Nq]
        vh = v.double().view(2, Nk, 3, 32).transpose(1, 2)                      # [B, H, Nk, 32]
        want = torch.gather(vh, 2, t[..., None].expand(-1, -1, -1, 32)).transpose(1, 2).reshape(2, Nq, 96)
        assert (ex.out - want).abs().max() < 1e-9
        dot = (q.double().view(2, Nq, 3, 32).transpose(1, 2) @ k.double().view(2, Nk, 3, 32).transpose(1, 2).transpose(-1, -2))
        assert (dot == dot.round()).all() and (dot.max(-1).values == 810).all()
        if Nk > 1:
            assert (dot.topk(2, -1).values[..., 1] <= 810 - 162).all()
    t = ab.routing_target(900, 1024, 2, 3)                                      # early and late chunks are both targeted
    assert (t < 128).any() and (t >= 896).any()


def test_window_routing_returns_the_target_token_or_the_region_mean():
    ws, shift, H, W = 12, 6, 13, 25
    qkv, qkv_bias, table = ab.window_routing(ws, shift, H, W, F16)
    ex = ab.exact_window(qkv, qkv_bias, table, H, W, 3, ws, shift)
    C = 96
    v = qkv.double().view(2, H, W, 3 * C)[..., 2 * C:]
    out = ex.out.view(2, H, W, C)
    # head 0 looks at its right-hand neighbour: an interior token (same window, same region) returns that token's v
    y, x = 2, 3
    assert (out[:, y, x, :32] - v[:, y, x + 1, :32]).abs().max() < 1e-9
    # head 1 at the token above ... (offset yi - yj = 1)
    assert (out[:, y, x, 32:64] - v[:, y - 1, x, 32:64]).abs().max() < 1e-9
    # the last real column's right-hand neighbour is a pad token: the bias
    assert (out[:, y, W - 1, :32] - qkv_bias.double()[2 * C:2 * C + 32]).abs().max() < 1e-9


def test_rel_index_is_the_models():
    from codetr.swin import WindowMSA

    for ws in (4, 7, 8, 12):
        assert torch.equal(ab.rel_index(ws), WindowMSA(32, 1, (ws, ws)).relative_position_index)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_graded_probability_sits_just_below_a_storage_step(dtype):
    """rounding moves the graded cases' p by < 0.1 of a storage step, truncation by 0.9 .. 0.98 of one: far enough from
    both neighbours that an fp32 ulp in the exponential cannot change either"""
    one = torch.tensor(1.0)
    p_dense = torch.exp2(0 - torch.tensor(ab.DENSE_GRADED_GAP[dtype], dtype=torch.float32) * ab.SCALE_LOG2E_F32)
    p_win = torch.exp2(ab._fma(torch.tensor(-ab.WINDOW_GRADED_GAP[dtype], dtype=torch.float32), ab.LOG2E_F32, 0 * one))
    for gap, p in ((ab.DENSE_GRADED_GAP[dtype], p_dense), (ab.WINDOW_GRADED_GAP[dtype], p_win)):
        assert torch.tensor(gap).to(dtype).item() == gap
        lo, hi = ab._to_storage(p, dtype, True), ab._to_storage(p, dtype, False)
        assert hi > lo and p >= 2.0 ** -14
        frac = ((p - lo) / (hi - lo)).item()
        assert 0.9 <= frac <= 0.98, frac
        assert ((p - lo) / p).item() > 1.5 * ab.U[dtype]


def test_non_finite_output_counts_as_wrong():
    q, k, v = ab.dense_uniform(1, F16)
    ex = ab.exact_mha(q, k, v, 3)
    assert ab.ratio(torch.full_like(ex.out, math.nan), ex, ab.structured_tol(ex)) == math.inf
