"""float64 references, derived error bounds, CPU emulations and test inputs for the two attention kernels (pure torch: the
same code runs on the CPU and on the device; tests/test_attention_bounds_cpu.py proves the bound and the cases,
tests/test_mha_attention_gpu.py and tests/test_window_attention_gpu.py run the kernels).

    dense   csrc/mha_attention.hip      softmax(q k^T / sqrt(32)) v, online softmax over 128-key chunks
    window  csrc/window_attention.hip   Swin (shifted-)window attention: pad tokens = qkv bias, roll, relative-position bias,
                                        literal -100 shift mask (reference codetr/swin.py:191-252, 92-112)

`exact_mha` / `exact_window` evaluate the formula in float64 on the 16-bit inputs and return an `Exact` (out, A, parts);
A = softmax . |v| is the absolute-value attention every relative term of the bound scales with.

`bound(exact)` -- where the kernels round.  u = storage unit roundoff (fp16 2^-11, bf16 2^-8); P = float64 softmax; p = the
kernel's probabilities (row max -> 1), l = their sum.

    u |exact| + tiny                the one rounding at the store (mha_attention.hip:175, window_attention.hip:349); tiny = half
                                    a step of the storage type below its normal range: fp16 2^-25; bf16 2^-126, where the
                                    fp32 product in front of the store may already be flushed
    u A                             p rounded to storage before P.V (mha_attention.hip:136, window_attention.hip:286); the
                                    dense kernel divides by the unrounded fp32 sum (:135, :140), the window kernel by the sum
                                    of the rounded p (:289): both first order u A
    2^-25 sum_j |v_j| [p_j < 2^-14] / l      fp16 only: half a step of a subnormal p (same lines).  In the dense kernel p is
                                    taken against the running max, which is not above the final one: a p that is subnormal there
                                    is subnormal here, and the later rescale (:146) is <= 1
    2 (P o (g + g_rowmax)) |v|      fp32 score error.  g[query, key] = 34 x 2^-24 x scale x sum_d |q_d| |k_d|: the 32 products
                                    of the MFMA (mha_attention.hip:111, window_attention.hip:228) plus the scale and log2 e
                                    multiplies (:115 / :251, :285); a relative error g of p_j moves the output by at most
                                    P_j g |v_j| directly and as much again through the sum.  The window kernel adds
                                    WIN_ROUNDINGS x 2^-24 x (|bias| + 100 [masked] + |logit|): the fmaf at :251, the subtraction
                                    at :252, the rounded log2 e and -mx log2 e (:271) and the fmaf at :285 -- at most four
                                    roundings of a quantity below that sum for a key and five for the row max
    2^-20 A                         v_exp_f32 and v_rcp_f32 (1 ulp each), the accumulation order of P.V and of the row sum
    2^-126 sum_j |v_j| / l          a p below the fp32 normal range is flushed (v_exp_f32): bf16 stores what fp16 would drop

`structured_tol(exact)` = u |exact| (1 + 2^-6) + tiny + 2^-20 A: for inputs whose probabilities are exactly 0, 1 or all equal, where
the u A term does not apply.

`emulate_mha` / `emulate_window` repeat the kernels' rounding points in fp32 torch (p cast to storage; row sum of the unrounded
p for the dense kernel, of the rounded p for the window kernel) and take `mutant=`, one of DENSE_MUTANTS / WINDOW_MUTANTS: the
errors the cases below exist to catch.

Inputs are drawn from a CPU generator (the same values on every machine) and moved to `device`.
"""
import collections
import math

import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -126}
HD = 32
SCALE = HD ** -0.5
CHUNK = 128                    # keys per online-softmax step of the dense kernel
MFMA_ROUNDINGS = 34            # 32 products + the scale and log2 e multiplies
WIN_ROUNDINGS = 5              # see the module docstring
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=torch.float32).item()
SCALE_F32 = torch.tensor(0.17677669529663687, dtype=torch.float32).item()
SCALE_LOG2E_F32 = (torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.tensor(32.0, dtype=torch.float32).sqrt()).item()

DENSE_MUTANTS = ("drop_last_key", "pads_counted", "swap_v_rows", "truncate_p")
WINDOW_MUTANTS = DENSE_MUTANTS + ("wrong_region_one_key", "pad_token_reads_zero", "bias_row_shifted")

Exact = collections.namedtuple("Exact", "out A parts")
Bound = collections.namedtuple("Bound", "total fp32")


# ------------------------------------------------------------------------------------------------------- float64
def _split_heads(t, H, dt):
    B, N, _ = t.shape
    return t.to(dt).reshape(B, N, H, HD).transpose(1, 2)


def _merge_heads(o):
    B, H, N, _ = o.shape
    return o.transpose(1, 2).reshape(B, N, H * HD)


def _exact(q, k, v, add, masked, merge, dtype, win):
    """q, k, v float64 [.., N, 32]; add: float64 bias or None; masked: bool or None"""
    dot = q @ k.transpose(-1, -2)
    logit = dot * SCALE
    g = MFMA_ROUNDINGS * 2.0 ** -24 * SCALE * (q.abs() @ k.abs().transpose(-1, -2))
    if win:
        mag = logit.abs() + add.abs()
        logit = logit + add
        if masked is not None:
            logit = logit - 100.0 * masked
            mag = mag + 100.0 * masked
        g = g + WIN_ROUNDINGS * 2.0 ** -24 * mag
    P = torch.softmax(logit, -1)
    out, A = P @ v, P @ v.abs()
    parts = {"P": P, "logit": logit, "g": g, "absv": v.abs(), "out": out, "A": A, "merge": merge, "dtype": dtype}
    return Exact(merge(out), merge(A), parts)


def exact_mha(q, k, v, H):
    """q [B, Nq, C], k, v [B, Nk, C] 16-bit -> Exact with out, A [B, Nq, C] float64"""
    f = torch.float64
    return _exact(_split_heads(q, H, f), _split_heads(k, H, f), _split_heads(v, H, f), None, None, _merge_heads, q.dtype, False)


def rel_index(ws, device="cpu"):
    """[N, N] row of the bias table for (query i, key j): offset (yi - yj + ws - 1, xi - xj + ws - 1) (WindowMSA's buffer)"""
    c = torch.stack(torch.meshgrid(torch.arange(ws, device=device), torch.arange(ws, device=device), indexing="ij")).flatten(1)
    rel = c[:, :, None] - c[:, None, :]
    return (rel[0] + ws - 1) * (2 * ws - 1) + (rel[1] + ws - 1)


def gather_bias(table, ws):
    """table [(2 ws - 1)^2, nH] -> [nH, N, N] (what WindowMSA.relative_position_bias() hands to the kernel)"""
    N = ws * ws
    return table[rel_index(ws, table.device).view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()


def _windows(qkv, qkv_bias, H, W, nH, ws, shift, dt, pad_zero=False):
    """The reference's pad (pad tokens = qkv(0) = the bias), roll and window partition.
    -> q, k, v [B nW, nH, N, 32] in `dt`, region ids [nW, N] (None without shift), merge(o) -> [B, H W, C]"""
    B, L, C3 = qkv.shape
    C = C3 // 3
    x = qkv.to(dt).view(B, H, W, C3)
    pad_b, pad_r = (-H) % ws, (-W) % ws
    Hp, Wp = H + pad_b, W + pad_r
    fill = torch.zeros(C3, dtype=dt, device=qkv.device) if pad_zero else qkv_bias.to(dt)
    full = fill.view(1, 1, 1, C3).expand(B, Hp, Wp, C3).clone()
    full[:, :H, :W] = x
    region = None
    if shift > 0:
        full = torch.roll(full, (-shift, -shift), (1, 2))
        reg = torch.zeros(Hp, Wp, device=qkv.device)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                reg[hs, wsl] = cnt
                cnt += 1
        region = reg.view(Hp // ws, ws, Wp // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    N = ws * ws
    win = full.view(B, Hp // ws, ws, Wp // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, C3)
    q, k, v = win.view(-1, N, 3, nH, HD).permute(2, 0, 3, 1, 4)

    def merge(o):
        o = o.transpose(1, 2).reshape(-1, N, C)
        o = o.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
        if shift > 0:
            o = torch.roll(o, (shift, shift), (1, 2))
        return o[:, :H, :W].reshape(B, H * W, C)

    return q, k, v, region, merge


def _masked(region, B):
    """[B nW, 1, N, N] bool: key in another shift-mask region than the query"""
    if region is None:
        return None
    m = region[:, None, :] != region[:, :, None]
    return m.repeat(B, 1, 1)[:, None]


def exact_window(qkv, qkv_bias, table, H, W, nH, ws, shift):
    """qkv [B, H W, 3C], qkv_bias [3C], table [(2 ws - 1)^2, nH] (all 16-bit) -> Exact with out, A [B, H W, C] float64"""
    f = torch.float64
    q, k, v, region, merge = _windows(qkv, qkv_bias, H, W, nH, ws, shift, f)
    m = _masked(region, qkv.shape[0])
    return _exact(q, k, v, gather_bias(table.to(f), ws)[None], None if m is None else m.to(f), merge, qkv.dtype, True)


def bound(ex):
    """Bound(total, fp32): the derived elementwise bound on |kernel - ex.out| and the part of it that fp32 arithmetic owns"""
    p = ex.parts
    u = U[p["dtype"]]
    logit, P, absv = p["logit"], p["P"], p["absv"]
    mx, arg = logit.max(-1, keepdim=True)
    pk = torch.exp(logit - mx)
    l = pk.sum(-1, keepdim=True)
    W = P * (p["g"] + p["g"].gather(-1, arg))
    fp32 = (2.0 * (W @ absv)                                   # scores: mha :111 :115 :134, window :228 :251 :252 :271 :285
            + 2.0 ** -20 * p["A"]                              # v_exp_f32, v_rcp_f32, accumulation order: mha :134 :169, window :285 :343
            + 2.0 ** -126 * absv.sum(-2, keepdim=True) / l)    # p flushed below the fp32 normal range: mha :134, window :285
    total = (u * p["out"].abs() + TINY[p["dtype"]]             # the store: mha :175, window :349
             + u * p["A"]                                      # p cast to storage: mha :136, window :286
             + fp32)
    if p["dtype"] == torch.float16:                            # half a step of a subnormal p: mha :136, window :286
        total = total + 2.0 ** -25 * ((pk < 2.0 ** -14).to(absv.dtype) @ absv) / l
    return Bound(p["merge"](total), p["merge"](fp32))


def structured_tol(ex):
    dtype = ex.parts["dtype"]
    return U[dtype] * ex.out.abs() * (1 + 2.0 ** -6) + TINY[dtype] + 2.0 ** -20 * ex.A


def ratio(got, ex, tol):
    """largest |got - exact| / tol; a non-finite output counts as infinitely wrong"""
    err = (got.double() - ex.out).abs()
    if not torch.isfinite(err).all():
        return math.inf
    return (err / tol).max().item()


# ------------------------------------------------------------------------------------------------------- emulations
def _to_storage(p, dtype, truncate):
    """fp32 p >= 0 -> the storage type and back (round to nearest even; or toward zero)"""
    if not truncate:
        return p.to(dtype).float()
    if dtype == torch.bfloat16:
        return (p.view(torch.int32) & -65536).view(torch.float32)
    h = p.half()
    h = (h.view(torch.int16) - (h.float() > p).to(torch.int16)).view(torch.float16)
    return h.float()


def _fma(a, b, c):
    """one fp32 rounding of a b + c"""
    return (a.double() * b + c.double()).float()


def emulate_mha(q, k, v, H, mutant=None):
    assert mutant is None or mutant in DENSE_MUTANTS
    dtype, f = q.dtype, torch.float32
    qh, kh, vh = (_split_heads(t, H, f) for t in (q, k, v))
    Nk = kh.shape[-2]
    NP = (Nk + 31) // 32 * 32
    if mutant == "swap_v_rows" and Nk > 1:
        perm = torch.arange(Nk)
        perm[Nk // 2], perm[Nk // 2 - 1] = Nk // 2 - 1, Nk // 2
        vh = vh[..., perm, :]
    pad = (0, 0, 0, NP - Nk)
    kh, vh = torch.nn.functional.pad(kh, pad), torch.nn.functional.pad(vh, pad)          # zero-filled K / V image rows
    t = (qh @ kh.transpose(-1, -2)) * SCALE_LOG2E_F32
    n_valid = NP if mutant == "pads_counted" else (Nk - 1 if mutant == "drop_last_key" else Nk)
    t[..., n_valid:] = -math.inf
    lead = t.shape[:-1]
    m_run = torch.full(lead + (1,), -math.inf, dtype=f, device=t.device)
    l_run = torch.zeros(lead + (1,), dtype=f, device=t.device)
    o = torch.zeros(lead + (HD,), dtype=f, device=t.device)
    for c0 in range(0, NP, CHUNK):
        tc = t[..., c0:c0 + CHUNK]
        m_new = torch.maximum(m_run, tc.max(-1, keepdim=True).values)
        corr = torch.exp2(m_run - m_new)
        p = torch.exp2(tc - m_new)
        l_run = l_run * corr + p.sum(-1, keepdim=True)
        o = o * corr + _to_storage(p, dtype, mutant == "truncate_p") @ vh[..., c0:c0 + CHUNK, :]
        m_run = m_new
    return _merge_heads((o * (1.0 / l_run)).to(dtype))


def emulate_window(qkv, qkv_bias, table, H, W, nH, ws, shift, mutant=None):
    assert mutant is None or mutant in WINDOW_MUTANTS
    dtype, f = qkv.dtype, torch.float32
    q, k, v, region, merge = _windows(qkv, qkv_bias, H, W, nH, ws, shift, f, pad_zero=mutant == "pad_token_reads_zero")
    N = ws * ws
    NP = (N + 15) // 16 * 16
    if mutant == "wrong_region_one_key" and region is not None:
        region = region.clone()
        region[:, N - 1] = 0
    if mutant == "swap_v_rows":
        perm = torch.arange(N)
        perm[N // 2], perm[N // 2 - 1] = N // 2 - 1, N // 2
        v = v[..., perm, :]
    bias = gather_bias(table.to(f), ws)[None]
    if mutant == "bias_row_shifted":
        bias = torch.roll(bias, -1, 2)
    x = _fma(q @ k.transpose(-1, -2), SCALE_F32, bias.expand(q.shape[0], -1, -1, -1))
    m = _masked(region, qkv.shape[0])
    if m is not None:
        x = torch.where(m, x - 100.0, x)
    if mutant == "drop_last_key":
        x[..., N - 1] = -math.inf
    if mutant == "pads_counted" and NP > N:            # zero rows of the K / V image: score 0, bias 0, v 0
        x = torch.nn.functional.pad(x, (0, NP - N))
        v = torch.nn.functional.pad(v, (0, 0, 0, NP - N))
    mx = x.max(-1, keepdim=True).values
    p = torch.exp2(_fma(x, LOG2E_F32, -mx * LOG2E_F32))
    pr = _to_storage(p, dtype, mutant == "truncate_p")
    o = (pr @ v) * (1.0 / pr.sum(-1, keepdim=True))
    return merge(o.to(dtype))


# ------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dense_random(B, Nq, Nk, H, dtype, seed, device="cpu", q_scale=1.0):
    g, C = _gen(seed), H * HD
    q = torch.randn(B, Nq, C, generator=g).to(dtype) * q_scale
    k, v = (torch.randn(B, Nk, C, generator=g).to(dtype) for _ in range(2))
    return q.to(device), k.to(device), v.to(device)


# (B, N, H) of the random self-attention cases: the decoder shape, key counts around the 128-key chunk and the 32-row padding
DENSE_RANDOM = [(2, 900, 8), (1, 1, 1), (1, 17, 2), (3, 127, 4), (1, 128, 8), (1, 129, 8), (1, 1000, 8), (1, 1024, 2)]
DENSE_UNIFORM_NK = [1, 31, 32, 33, 97, 127, 129, 255, 257, 897, 1023, 1024]
DENSE_ROUTING = [(1, 1), (17, 33), (129, 127), (300, 900), (900, 1024)]
DENSE_ROUTING_FUSED = (900, 900)      # run with q | k as the column halves of one [B, N, 2C] tensor
DENSE_GRADED = [(17, 33), (129, 127), (300, 900)]
# score gap (in q . k units) between the one leading key and the rest of a graded case, per type: p = exp(-gap / sqrt(32)) lies
# 0.9 .. 0.98 of a storage step above a representable value near the bottom of its binade, so that rounding moves it by < 0.1
# step and truncation by > 0.9 (tests/test_attention_bounds_cpu.py checks that position)
DENSE_GRADED_GAP = {torch.float16: 3.25, torch.bfloat16: 7.5}


def dense_uniform(Nk, dtype, device="cpu", Nq=17, B=2, H=3):
    """q = 0: every row is the mean of v over exactly the Nk real keys; the last key's row is 32"""
    g, C = _gen(Nk), H * HD
    q = torch.zeros(B, Nq, C, dtype=dtype)
    k = torch.randn(B, Nk, C, generator=g).to(dtype)
    v = torch.randint(-3, 4, (B, Nk, C), generator=g).to(dtype)
    v[:, -1] = 32
    return q.to(device), k.to(device), v.to(device)


def routing_target(Nq, Nk, B, H):
    """[B, H, Nq]: the key that query i of (b, h) must return"""
    i = torch.arange(Nq).view(1, 1, Nq)
    return (389 * i + 7 + 101 * torch.arange(H).view(1, H, 1) + 13 * torch.arange(B).view(B, 1, 1)) % Nk


def _code(j):
    """+-9 binary code of j in 10 dims"""
    bits = (j[..., None] >> torch.arange(10)) & 1
    return (bits * 18 - 9).float()


def dense_routing(Nq, Nk, dtype, device="cpu", B=2, H=3):
    """q . k is an exact integer, 810 at the target and at most 810 - 162 elsewhere: the row is v[target]"""
    g, C = _gen(1000 * Nq + Nk), H * HD
    k = torch.randn(B, Nk, H, HD, generator=g)
    k[..., :10] = _code(torch.arange(Nk)).view(1, Nk, 1, 10)
    q = torch.zeros(B, Nq, H, HD)
    q[..., :10] = _code(routing_target(Nq, Nk, B, H)).permute(0, 2, 1, 3)
    v = torch.randn(B, Nk, C, generator=g)
    return q.view(B, Nq, C).to(dtype).to(device), k.view(B, Nk, C).to(dtype).to(device), v.to(dtype).to(device)


def graded_leader(Nk, B, H):
    """[B, H]: the leading key of (b, h), inside the first 128-key chunk so that every other key is taken against its max"""
    return (7 + 101 * torch.arange(H).view(1, H) + 13 * torch.arange(B).view(B, 1)) % min(Nk, CHUNK)


def dense_graded(Nq, Nk, dtype, device="cpu", B=2, H=3):
    """Two score levels: one leading key per (b, h) with v = 0, every other key `gap` below it with positive integer v.  The
    output is all rounded probability: p sum(v) / (1 + (Nk - 1) p)."""
    g, C = _gen(7 * Nq + Nk), H * HD
    q = torch.zeros(B, Nq, H, HD)
    q[..., 0] = 1
    k = torch.zeros(B, Nk, H, HD)
    v = torch.randint(1, 8, (B, Nk, H, HD), generator=g).float()
    lead = graded_leader(Nk, B, H)
    for b in range(B):
        for h in range(H):
            k[b, lead[b, h], h, 0] = DENSE_GRADED_GAP[dtype]
            v[b, lead[b, h], h] = 0
    return tuple(t.view(t.shape[0], t.shape[1], C).to(dtype).to(device) for t in (q, k, v))


# (B, H, W, nH, ws, shift, seed, bias_scale, dtype) of the random window cases (what the three parametrised tests and the large-
# bias test of tests/test_window_attention_gpu.py run)
def window_random_cases():
    f, b = torch.float16, torch.bfloat16
    cases = []
    for shift in (0, 6):
        for B, H, W, nH in [(1, 12, 12, 1), (2, 24, 36, 2), (1, 20, 31, 6), (3, 13, 12, 3), (1, 40, 60, 4)]:
            cases.append((B, H, W, nH, 12, shift, H + W + shift, 1.0, f))
    for ws, shift, H, W in [(7, 0, 14, 14), (7, 3, 16, 20), (8, 4, 17, 9), (4, 2, 11, 15), (4, 0, 8, 8)]:
        cases.append((2, H, W, 2, ws, shift, ws, 1.0, f))
    for ws, shift, B, H, W, nH in [(12, 0, 2, 24, 36, 2), (12, 6, 1, 20, 31, 6), (7, 3, 2, 16, 20, 2), (12, 6, 1, 40, 60, 4)]:
        cases.append((B, H, W, nH, ws, shift, ws + H, 1.0, b))
    cases.append((1, 30, 30, 2, 12, 6, 9, 8.0, f))
    return cases


def window_random(B, H, W, nH, ws, shift, seed, bias_scale, dtype, device="cpu"):
    """-> qkv [B, H W, 3C], qkv_bias [3C], table [(2 ws - 1)^2, nH]"""
    g, C = _gen(seed), nH * HD
    qkv = torch.randn(B, H * W, 3 * C, generator=g).to(dtype)
    qkv_bias = (0.5 * torch.randn(3 * C, generator=g)).to(dtype)
    table = (bias_scale * torch.randn((2 * ws - 1) ** 2, nH, generator=g)).to(dtype)
    return qkv.to(device), qkv_bias.to(device), table.to(device)


# (ws, shift, H, W): one window with four regions; pads both ways; no shift; N = 49 (the key-tail branch); two small windows
WINDOW_STRUCTURED = [(12, 6, 12, 12), (12, 6, 13, 25), (12, 0, 24, 36), (7, 3, 16, 20), (8, 4, 17, 9), (4, 2, 11, 15)]
WINDOW_GRADED = [(12, 6, 13, 25), (7, 3, 16, 20), (8, 4, 17, 9)]
# the bias of every relative offset but one in a graded case is -WINDOW_GRADED_GAP (16-bit exact): p = exp(-gap), placed like
# DENSE_GRADED_GAP
WINDOW_GRADED_GAP = {torch.float16: 7.5, torch.bfloat16: 8.25}


def window_uniform(ws, shift, H, W, dtype, device="cpu", B=2, nH=3):
    """q = 0 and a zero table: every query returns the mean of v over its own shift-mask region of its window; pad tokens
    (v = the bias = 16) show in it"""
    g, C = _gen(100 * ws + H), nH * HD
    qkv = torch.randn(B, H * W, 3 * C, generator=g)
    qkv[..., :C] = 0
    qkv[..., 2 * C:] = torch.randint(-3, 4, (B, H * W, C), generator=g).float()
    qkv_bias = 0.5 * torch.randn(3 * C, generator=g)
    qkv_bias[:C] = 0
    qkv_bias[2 * C:] = 16
    table = torch.zeros((2 * ws - 1) ** 2, nH)
    return qkv.to(dtype).to(device), qkv_bias.to(dtype).to(device), table.to(dtype).to(device)


def routing_offsets(ws):
    """(yi - yj, xi - xj) per head: a horizontal neighbour, a vertical neighbour, the far corner"""
    return [(0, -1), (1, 0), (ws - 1, -(ws - 1))]


def window_routing(ws, shift, H, W, dtype, device="cpu", B=2):
    """q = 0; head h's table is 48 at one relative offset and 0 elsewhere: a query whose target lies in its window and
    region returns that token's v (a pad token's: the bias), any other its region mean (48 - 100 loses)"""
    offs = routing_offsets(ws)
    nH = len(offs)
    g, C = _gen(100 * ws + W), nH * HD
    qkv = torch.randn(B, H * W, 3 * C, generator=g)
    qkv[..., :C] = 0
    qkv_bias = 0.5 * torch.randn(3 * C, generator=g)
    qkv_bias[:C] = 0
    table = torch.zeros((2 * ws - 1) ** 2, nH)
    for h, (dy, dx) in enumerate(offs):
        table[(dy + ws - 1) * (2 * ws - 1) + dx + ws - 1, h] = 48
    return qkv.to(dtype).to(device), qkv_bias.to(dtype).to(device), table.to(dtype).to(device)


def window_graded(ws, shift, H, W, dtype, device="cpu", B=2, nH=3):
    """q = 0; the table is 0 at the offset of the right-hand neighbour and -gap elsewhere; v is 0 in even columns and a positive
    integer in odd ones (pad tokens: 5).  A query in an odd column with its neighbour in reach returns
    p sum(v) / (1 + (n - 1) p) over its region: all rounded probability."""
    g, C = _gen(100 * ws + H + W), nH * HD
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    qkv[..., :C] = 0
    qkv[..., 2 * C:] = torch.randint(1, 8, (B, H, W, C), generator=g).float()
    qkv[:, :, 0::2, 2 * C:] = 0
    qkv_bias = 0.5 * torch.randn(3 * C, generator=g)
    qkv_bias[:C] = 0
    qkv_bias[2 * C:] = 5
    table = torch.full(((2 * ws - 1) ** 2, nH), -WINDOW_GRADED_GAP[dtype])
    table[(ws - 1) * (2 * ws - 1) + (-1) + ws - 1] = 0
    return qkv.view(B, H * W, 3 * C).to(dtype).to(device), qkv_bias.to(dtype).to(device), table.to(dtype).to(device)


def dense_strided(device="cpu"):
    """q | k as the column halves of one [2, 300, 512] projection, v, and a shorter query set (cross lengths)"""
    g = _gen(1)
    qk = torch.randn(2, 300, 512, generator=g).half()
    v = torch.randn(2, 300, 256, generator=g).half()
    q2 = torch.randn(2, 70, 256, generator=g).half()
    return qk.to(device), v.to(device), q2.to(device)


def dense_random_inputs(device="cpu"):
    """every random dense case the GPU module runs: (name, q, k, v, H, (rtol, atol) of the tolerance it replaced, unit_scale)"""
    f, b = torch.float16, torch.bfloat16
    for B, N, H in DENSE_RANDOM:
        yield (f"f16 B{B} N{N} H{H}",) + dense_random(B, N, N, H, f, N + H, device) + (H, (5e-3, 3e-3), True)
    qk, v, q2 = dense_strided(device)
    yield ("f16 strided 300x300", qk[..., :256], qk[..., 256:], v, 8, (5e-3, 3e-3), True)
    yield ("f16 strided 70x300", q2, qk[..., 256:], v, 8, (5e-3, 3e-3), True)
    yield ("f16 q x 30",) + dense_random(1, 400, 400, 2, f, 2, device, q_scale=30.0) + (2, (5e-3, 5e-3), False)
    yield ("bf16 B2 N333 H4",) + dense_random(2, 333, 333, 4, b, 3, device) + (4, (2e-2, 2e-2), True)


def window_legacy_tol(dtype):
    return (5e-3, 3e-3) if dtype == torch.float16 else (2e-2, 2e-2)
