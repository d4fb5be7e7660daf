"""The constructed epilogue cases of tests/epilogue_exact.py, checked without a GPU:

* every accumulator, every `acc + bias` and every `E(..) + r` of the cases is exact in fp32 (compared in float64), so the
  contract determines the output bits;
* `gelu_emulated` (device_prims.h's formula in fp32) against float64 0.5 x erfc(-x / sqrt 2): at most 2.4e-7 |x| absolute,
  the fp16 result within 2 ulp of the correctly rounded one and more than 1 ulp only for -6 < x < -3 -- which pins the
  coefficients and is what the header comment of gelu_erf now says;
* every wrong epilogue named in the contract's description changes outputs on these inputs (counts asserted), i.e. the
  GPU comparison would reject it.
"""
import math

import pytest
import torch

import epilogue_exact as ee

DTYPES = [torch.float16, torch.bfloat16]
F32_MAX = 3.4028234663852886e38
K = 64


def _sets(T):
    return {"A": ee.set_a(T, K, "cpu"), "B": ee.set_r(T, K, "cpu", bias_js=(0, 1, 2, 3), x_js=(0,)),
            "B2": ee.set_r(T, K, "cpu")}


@pytest.mark.parametrize("T", DTYPES)
def test_every_constructed_case_is_exact(T):
    for name, case in _sets(T).items():
        M = case["k1"].numel()
        a32, a64 = ee.accumulators(case, M), ee.accumulators(case, M, torch.float64)
        big = a64.abs() > F32_MAX
        assert bool((a32.double() == a64)[~big].all()) and bool(a32[big].isinf().all()), name
        assert name == "A" or not big.any()
        # no matrix-core operand is subnormal
        tiny = 2.0 ** (-14 if T == torch.float16 else -126)
        for t in (case["w"], ee.make_x(case, M)):
            assert bool(((t == 0) | (t.double().abs() >= tiny)).all()), name
        if case["b"] is not None:
            b = case["b"]
            fin = b.isfinite()
            p32, p64 = ee.pre_activation(a32, b), a64 + b.double()[None, :]
            assert bool((p32.double() == p64)[:, fin][~big[:, fin]].all()), name
        if name == "B2":
            lin = ee.pre_activation(a32, case["b"]).to(T)
            for mode in ("q", "cancel"):
                r = ee.residual(case, M, mode)
                assert bool(((lin.float() + r.float()).double() == lin.double() + r.double()).all()), (name, mode)


def test_set_a_covers_every_finite_fp16_pattern_and_the_results_between_subnormals():
    case = ee.set_a(torch.float16, K, "cpu", nonfinite_bias=False)
    M = case["k1"].numel()
    acc = ee.accumulators(case, M)
    got = torch.unique(acc.half().view(torch.int16).int() & 0xffff)
    finite = torch.tensor([b for b in range(65536) if (b & 0x7c00) != 0x7c00 and b != 0x8000])   # (-0 arrives as +0)
    assert set(finite.tolist()) <= set(got.tolist())
    assert 0x7c00 in got.tolist() and 0xfc00 in got.tolist()        # products that leave the fp16 range
    q = torch.unique((acc[K:2 * K].abs().double() * 2.0 ** 26).round())
    assert set(range(1, 2048)) <= set(q.long().tolist())             # q 2^-26, q = 1 .. 2047


def test_gelu_emulated_error_is_absolute_and_at_most_two_fp16_ulp():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    h = bits.view(torch.float16)
    x16 = h[h.isfinite()].float()
    bf = bits.view(torch.bfloat16).float()
    xbf = bf[(bf.abs() >= 2.0 ** -64) & (bf.abs() <= 2.0 ** 64)]
    worst = 0.0
    for x in (x16, xbf):
        err = (ee.gelu_emulated(x).double() - ee.gelu_ref64(x)).abs()
        nz = x != 0
        worst = max(worst, float((err[nz] / x.double().abs()[nz]).max()))
    assert worst <= ee.GELU_EMULATED_MAX, worst
    assert worst > 1.2e-7          # the claim the header made (< 2^-22 RELATIVE on the output) is not what holds:
    rel = (ee.gelu_emulated(x16).double() - ee.gelu_ref64(x16)).abs() / ee.gelu_ref64(x16).abs().clamp_min(1e-300)
    assert float(rel[x16 < -5].max()) >= 1.0      # ... the relative error reaches 100 % (the sign is lost) below -5
    # fp16: the rounded result against the correctly rounded one, in ulps (bit patterns of one sign are consecutive)
    got, want = ee.gelu_emulated(x16).half(), ee.gelu_ref64(x16).float().half()
    def key(v):
        b = v.view(torch.int16).int()
        return torch.where(b < 0, -(b & 0x7fff), b)
    d = (key(got) - key(want)).abs()
    assert int(d.max()) <= 2
    far = d > 1
    assert bool(((x16[far] > -6) & (x16[far] < -3)).all()), x16[far]
    assert int(far.sum()) <= 21


@pytest.mark.parametrize("T", DTYPES)
def test_wrong_epilogues_are_rejected(T):
    """set B2 (both quarter-ulp routes, bias in {0, ulp/4}, the three residuals) against: a truncating conversion, one
    rounding with the residual, the bias added after the rounding; set A under ReLU against a ReLU that maps NaN to 0"""
    case = ee.set_r(T, K, "cpu")
    M = case["k1"].numel()
    acc = ee.accumulators(case, M)
    counts = {"trunc": 0, "single_round": 0, "bias_after": 0}
    total = 0
    for b in (None, case["b"]):
        for mode in (None, "q", "cancel"):
            r = ee.residual(case, M, mode) if mode else None
            want = ee.expected(acc, b, r, None, T)
            total += want.numel()
            for m in counts:
                counts[m] += ee.differing(ee.expected(acc, b, r, None, T, mutate=m), want)
    a = ee.set_a(T, K, "cpu")
    Ma = a["k1"].numel()
    acca = ee.accumulators(a, Ma)
    counts["relu_nan0"] = ee.differing(ee.expected(acca, a["b"], None, "relu", T, mutate="relu_nan0"),
                                       ee.expected(acca, a["b"], None, "relu", T))
    print(T, total, counts)
    assert counts == EXPECTED_COUNTS[T], (total, counts)
    assert all(v > 0 for v in counts.values())


@pytest.mark.parametrize("T", DTYPES)
def test_wrong_gelus_are_rejected(T):
    case = ee.set_a(T, K, "cpu")
    M = case["k1"].numel()
    z = ee.pre_activation(ee.accumulators(case, M), case["b"])
    ok, _ = ee.gelu_accept(ee.gelu_emulated(z).to(T), z, T)
    assert bool(ok.all()), int((~ok).sum())                 # the formula itself passes
    clamped = int((~ee.gelu_accept(ee.gelu_clamped(z).to(T), z, T)[0]).sum())
    tanh = int((~ee.gelu_accept(ee.gelu_tanh(z).to(T), z, T)[0]).sum())
    print(T, clamped, tanh)
    assert (clamped, tanh) == EXPECTED_GELU_COUNTS[T]
    assert clamped > 0 and tanh > 0


# outputs each wrong epilogue changes, of 2 776 032 (fp16) / 2 322 432 (bf16) rounding cases (set B2 x bias {0, ulp/4} x
# residual {none, 3/8 ulp, -0.75 v}) and, for the ReLU, of set A's NaN outputs; integer-exact on any CPU
EXPECTED_COUNTS = {
    torch.float16: {"trunc": 1040694, "single_round": 1040266, "bias_after": 173502, "relu_nan0": 192},
    torch.bfloat16: {"trunc": 869376, "single_round": 867328, "bias_after": 145152, "relu_nan0": 128},
}
# set A outputs outside the GELU interval: (GELU clamped to 0 below -3, tanh-form GELU)
EXPECTED_GELU_COUNTS = {torch.float16: (2020, 7264), torch.bfloat16: (381, 398)}
