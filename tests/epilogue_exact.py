"""Exact inputs and the bit-for-bit contract of the GEMM epilogues (pure torch: the same code runs on the CPU and on the
device; tests/test_epilogue_exact_cpu.py checks the construction, tests/test_epilogue_exact_gpu.py runs the kernels).

The contract lives in csrc/gemm_epilogue.h, the header the GEMM kernels of csrc/gemm_tile128.hip, csrc/gemm_tile256.hip, csrc/gemm_xs.hip, csrc/gemm_persist.h and
csrc/gemm_fp8.hip take their output values from (csrc/ffn_fused.hip states its own, for its second product):

    y = E(E(act(acc + bias)) + r)            E = ONE round-to-nearest-even to the storage type
    act 3 ("relu_res"):  y = E(relu(E(acc + bias) + r))
    row state 1: the linear output is 0 (+ r);  row state 2: it is E(act(bias)) (+ r)

A GEMM whose x rows are one-hot reproduces chosen pre-activations with no accumulation error, so the output is determined
bit for bit.  A *case* (dict) describes such a GEMM:

    w   [N, K]  storage type         b  [N] storage type or None        q [N] storage type (the residual 3/8 ulp, set R)
    k1, a1 [M0]: row m holds a1[m] at column k1[m];   k2, a2 [M0] (optional): a second non-zero
    -> acc[m, n] = a1[m] w[n, k1[m]] + a2[m] w[n, k2[m]]     (every product and the sum exact in fp32)

Rows repeat with period M0 when a kernel needs more rows.  No matrix-core operand is subnormal: subnormal fp16 results come
from the row scale 2^-13.

* set A (values): w enumerates every normal pattern of the type (fp16: all; bf16: 2^-64 <= |v| <= 2^64) and +-0, the rows
  scale it by 1, 2^-13 (fp16: every subnormal pattern v = 2^-13 x (v 2^13), and every q 2^-26, q = 1 .. 2047: results between
  the subnormals) and 60000 (products that leave the fp16 range); bf16: 1 and 181/128 x 2^64 (products that round to inf in
  bf16, or leave fp32).  +inf, -inf and NaN enter through the bias of three columns whose weights are zero.
* set R (rounding): a column holds the mantissas of one binade and sign; z = v + s j ulp(v) / 4, j = 0 .. 3, the quarter
  ulps either from the bias (`bias_js`) or from a second product a2 w[n, K - 1] = (j 2^-(p+2)) x (s 2^e) (`x_js`).
"""
import math

import torch

P = {torch.float16: 10, torch.bfloat16: 7}            # explicit mantissa bits
A_RANGE = {torch.float16: (-14, 15), torch.bfloat16: (-64, 63)}      # binades of set A (bf16: + the value 2^64)
R_RANGE = {torch.float16: (-11, 15), torch.bfloat16: (-64, 63)}      # binades of set R
GELU_C = 4.8e-7          # |gelu_erf(z) - gelu(z)| <= GELU_C |z|: 2.4e-7 (the fp32 formula, measured by the CPU test) + 2.4e-7
#                          (v_rcp_f32 and v_exp_f32 are 1-ulp operations: 0.5 x 3 x 2^-23 = 1.8e-7 derived)
GELU_EMULATED_MAX = 2.4e-7


def _cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------- the cases
def values_a(T, device):
    """float64 [n]: every value of set A"""
    p, (e0, e1) = P[T], A_RANGE[T]
    e = torch.arange(e0, e1 + 1, dtype=torch.float64, device=device)
    m = torch.arange(2 ** p, dtype=torch.float64, device=device)
    mag = (torch.exp2(e)[:, None] * (1 + m / 2 ** p)[None, :]).flatten()
    extra = [0.0, -0.0] + ([2.0 ** 64, -2.0 ** 64] if T == torch.bfloat16 else [])
    return torch.cat((mag, -mag, torch.tensor(extra, dtype=torch.float64, device=device)))


def row_scales_a(T):
    return [1.0, 2.0 ** -13, 60000.0] if T == torch.float16 else [1.0, 181.0 / 128 * 2.0 ** 64]


def set_a(T, K, device, nonfinite_bias=True, scales=None):
    v = values_a(T, device)
    ncol = _cdiv(v.numel(), K)
    w = torch.zeros(ncol * K, dtype=torch.float64, device=device)
    w[:v.numel()] = v
    w = w.view(ncol, K)
    b = None
    if nonfinite_bias:
        w = torch.cat((w, torch.zeros(3, K, dtype=torch.float64, device=device)))
        b = torch.zeros(ncol + 3, dtype=torch.float64, device=device)
        b[ncol:] = torch.tensor([math.inf, -math.inf, math.nan], dtype=torch.float64, device=device)
        b = b.to(T)
    scales = row_scales_a(T) if scales is None else scales
    k1 = torch.arange(K, device=device).repeat(len(scales))
    a1 = torch.tensor(scales, dtype=torch.float64, device=device).repeat_interleave(K).to(T)
    return {"T": T, "w": w.to(T), "b": b, "q": None, "k1": k1, "a1": a1, "k2": None, "a2": None}


def set_r(T, K, device, bias_js=(0, 1), x_js=(0, 1, 2, 3), p_out=None):
    """p_out: mantissa bits of the type the result is rounded to (codetr_linear_bf16_f16out: bf16 operands, fp16 result)"""
    p = P[T]
    po = p if p_out is None else p_out
    e0, e1 = R_RANGE[T if p_out is None else torch.float16]
    kc, L = K - 1, 2 ** p
    nch = _cdiv(L, kc)
    mant = (torch.arange(nch * kc, device=device) % L).view(nch, kc).double()
    e = torch.arange(e0, e1 + 1, dtype=torch.float64, device=device)
    s = torch.tensor([1.0, -1.0], dtype=torch.float64, device=device)
    jb = torch.tensor(bias_js, dtype=torch.float64, device=device)
    ch = torch.arange(nch, device=device)
    ge, gs, gj, gc = [g.flatten() for g in torch.meshgrid(e, s, jb, ch.double(), indexing="ij")]
    lead = gs * torch.exp2(ge)                                   # s 2^e per column
    w = torch.empty(ge.numel(), K, dtype=torch.float64, device=device)
    w[:, :kc] = lead[:, None] * (1 + mant[gc.long()] / L)
    w[:, kc] = lead
    b = (lead * gj * 2.0 ** -(po + 2) + 0.0).to(T) if any(bias_js) else None      # (+ 0: a zero bias is +0)
    q = (lead * 3 * 2.0 ** -(po + 3)).to(T)
    nj = len(x_js)
    k1 = torch.arange(kc, device=device).repeat(nj)
    a1 = torch.ones(kc * nj, dtype=T, device=device)
    k2 = torch.full((kc * nj,), kc, device=device)
    a2 = (torch.tensor(x_js, dtype=torch.float64, device=device) * 2.0 ** -(po + 2)).repeat_interleave(kc).to(T)
    return {"T": T, "w": w.to(T), "b": b, "q": q, "k1": k1, "a1": a1, "k2": k2, "a2": a2}


def pad_columns(case, N):
    """the case with N >= its columns: zero weights, zero bias"""
    c = dict(case)
    n0 = case["w"].shape[0]
    assert N >= n0
    if N == n0:
        return c
    c["w"] = torch.cat((case["w"], case["w"].new_zeros(N - n0, case["w"].shape[1])))
    for key in ("b", "q"):
        if case[key] is not None:
            c[key] = torch.cat((case[key], case[key].new_zeros(N - n0)))
    return c


def take_columns(case, lo, hi):
    c = dict(case)
    for key in ("w", "b", "q"):
        if case[key] is not None:
            c[key] = case[key][lo:hi].contiguous()
    return c


def rows(case, M):
    """index of the case row behind each of M GEMM rows"""
    return torch.arange(M, device=case["w"].device) % case["k1"].numel()


def make_x(case, M):
    w = case["w"]
    idx = rows(case, M)
    x = torch.zeros(M, w.shape[1], dtype=w.dtype, device=w.device)
    ar = torch.arange(M, device=w.device)
    x[ar, case["k1"][idx]] = case["a1"][idx]
    if case["k2"] is not None:
        x[ar, case["k2"][idx]] = case["a2"][idx]
    return x


def accumulators(case, M, dtype=torch.float32):
    """acc [M, N] in `dtype`: float32 is what the matrix cores hold, float64 what the CPU test compares it with.  The
    accumulators start at +0, so a product of -0 arrives as +0 (the `+ 0`)."""
    idx = rows(case, M)
    wt = case["w"].to(dtype).t()
    acc = case["a1"][idx].to(dtype)[:, None] * wt[case["k1"][idx]]
    if case["k2"] is not None:
        acc = acc + case["a2"][idx].to(dtype)[:, None] * wt[case["k2"][idx]]
    return acc + 0.0


def residual(case, M, mode):
    """mode 'q': s 3 ulp / 8 of the column; 'cancel': -0.75 v rounded to the type; 'mix': row blocks of the two"""
    T = case["w"].dtype
    idx = rows(case, M)
    rq = case["q"][None, :].expand(M, -1)
    if mode == "q":
        return rq.contiguous()
    rc = (-0.75 * case["w"].float().t()[case["k1"][idx]]).to(T)
    if mode == "cancel":
        return rc
    assert mode == "mix"
    return torch.where(((torch.arange(M, device=rq.device) // 8) % 2 == 0)[:, None], rq, rc).contiguous()


# ------------------------------------------------------------------------------------------------------- the contract
def round_rne(x32, T):
    return x32.to(T)


def round_trunc(x32, T):
    """(a mutation) round toward zero"""
    y = x32.to(T)
    over = y.float().abs() > x32.abs()          # (also a finite value rounded to inf)
    return torch.where(over, y.view(torch.int16) - 1, y.view(torch.int16)).view(T)


def relu_nan(x):
    """x < 0 ? 0 : x  (NaN propagates)"""
    return torch.where(x < 0, torch.zeros_like(x), x)


def pre_activation(acc, b, state=None):
    """acc + bias in fp32; rows of state 2 count as zero input rows"""
    if state is not None:
        acc = torch.where((state == 2)[:, None], torch.zeros_like(acc), acc)
    return acc + b.float()[None, :] if b is not None else acc


def expected(acc, b, r, act, T, state=None, mutate=None):
    """the contract in float32 torch ops; act in {None, 'relu', 'relu_res'} (GELU: gelu_accept).  mutate: one of the wrong
    epilogues the CPU test shows the cases reject -- 'trunc', 'single_round', 'bias_after', 'relu_nan0'"""
    E = round_trunc if mutate == "trunc" else round_rne
    relu = (lambda t: torch.relu(t).nan_to_num(nan=0.0, posinf=math.inf, neginf=-math.inf)) if mutate == "relu_nan0" else relu_nan
    if mutate == "bias_after" and b is not None:
        pre = E(pre_activation(acc, None, state), T).float() + b.float()[None, :]
    else:
        pre = pre_activation(acc, b, state)
    if act == "relu" or (act == "relu_res" and r is None):
        pre = relu(pre)
    if mutate == "single_round" and r is not None:
        lin = pre
    else:
        lin = E(pre, T).float()
    if state is not None:
        lin = torch.where((state == 1)[:, None], torch.zeros_like(lin), lin)
    if r is None:
        return E(lin, T)
    y = lin + r.float()
    if act == "relu_res":
        y = relu(y)
    return E(y, T)


def canonical_bits(y):
    """int16 bits with every NaN as one pattern (the payload of a NaN is not part of the contract)"""
    bits = y.view(torch.int16)
    return torch.where(y.isnan(), torch.full_like(bits, 0x7e00), bits)


def differing(y, want):
    return int((canonical_bits(y) != canonical_bits(want)).sum())


# --------------------------------------------------------------------------------------------------------------- GELU
def gelu_ref64(z32):
    z = z32.double()
    return 0.5 * z * torch.special.erfc(-z / math.sqrt(2.0))


def gelu_accept(y, z32, T, r=None, c=GELU_C):
    """-> (ok [bool, like y], excess): y is accepted iff it lies between E(ref - a) and E(ref + a), a = c |z| (pushed through
    E(. + r) with a residual: rounding is monotone); a non-finite z must match fp32 F.gelu on the CPU in NaN-ness and in the
    sign of inf.  excess = max over finite z of (|y - ref| - half an ulp of the result - what a residual adds) / |z|: the part
    of the error that the output rounding cannot explain, i.e. a lower bound on the error of the fp32 formula as run."""
    z = z32.double()
    ref = gelu_ref64(z32)
    a = c * z.abs()
    fin = z32.isfinite()
    lo, hi = (ref - a).float().to(T), (ref + a).float().to(T)
    if r is not None:
        lo, hi = (lo.float() + r.float()).to(T), (hi.float() + r.float()).to(T)
    yf = y.float()
    ok = (yf >= lo.float()) & (yf <= hi.float())
    if (~fin).any():
        # one element at a time: the vectorised fp32 CPU kernel of some torch builds returns NaN for +inf where its own
        # scalar path (and float64) return +inf
        g1 = [float(torch.nn.functional.gelu(torch.tensor([v], dtype=torch.float32))) for v in (math.inf, -math.inf)]
        zn = z32[~fin]
        g = torch.where(zn == math.inf, g1[0], torch.where(zn == -math.inf, g1[1], math.nan)).float()
        if r is not None:
            g = g + r.float()[~fin]
        yn = yf[~fin]
        ok[~fin] = (yn.isnan() == g.isnan()) & (g.isnan() | (yn == g))
    excess = 0.0
    if r is None:
        sel = fin & (z32 != 0) & yf.isfinite()
        if sel.any():
            yd = yf.double()[sel]
            # half an ulp of the result: spacing of T at |y| (at least the subnormal spacing)
            emin = -14 if T == torch.float16 else -126
            ex = torch.floor(torch.log2(yd.abs().clamp_min(2.0 ** emin)))
            half = torch.exp2(ex - P[T] - 1)
            excess = float((((yd - ref[sel]).abs() - half).clamp_min(0) / z.abs()[sel]).max())
    return ok, excess


def _c32(v):
    return torch.tensor(v, dtype=torch.float32)


def gelu_emulated(x32):
    """device_prims.h's gelu_erf in fp32, every step rounded once (float64 product-sum, then to fp32), the reciprocal and
    exp2 exact: what the formula itself gives, apart from the two 1-ulp hardware operations"""
    def fma(a, b, c):
        return (a.double() * b.double() + c.double()).float()

    def mul(a, b):
        return (a.double() * b.double()).float()

    dev = x32.device
    k = [_c32(v).to(dev) for v in (0.3275911, 0.70710678118654752, 1.061405429, -1.453152027, 1.421413741, -0.284496736,
                                   0.254829592, 1.4426950408889634)]
    half, one = _c32(0.5).to(dev), _c32(1.0).to(dev)
    u = x32.abs()
    t = (1.0 / fma(mul(k[0], k[1]), u, one).double()).float()
    p = fma(mul(half, k[2]), t, mul(half, k[3]))
    p = fma(p, t, mul(half, k[4]))
    p = fma(p, t, mul(half, k[5]))
    p = fma(p, t, mul(half, k[6]))
    ez = torch.exp2(mul(mul(u, u), mul(-half, k[7])).double()).float()
    return fma(u, fma(-mul(p, t), ez, half), mul(half, x32))


def gelu_clamped(z32):
    """(a mutation) GELU that returns 0 below -3"""
    return torch.where(z32 < -3, torch.zeros_like(z32), gelu_ref64(z32).float())


def gelu_tanh(z32):
    """(a mutation) the tanh form"""
    return torch.nn.functional.gelu(z32.double(), approximate="tanh").float()
