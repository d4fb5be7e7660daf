"""float64 references, derived interval bounds, launch plans, CPU emulations and test inputs for the two fused MLP kernels (pure
torch: the same code runs on the CPU and on the device; tests/test_ffn_bounds_cpu.py proves the bounds, the cases and the plans,
tests/test_ffn_gpu.py and tests/test_swin_mlp_gpu.py run the kernels).

    ffn        csrc/ffn_fused.hip   [oproj] x0 = E(E(Wo a + bo) + identity)   [ln_in] x1 = E(LN_in(x0))
                                    h = relu(E(W1 x1 + b1))   y = E(W2 h + b2)   t = E(y + x1)   [ln] Y = E(LN(t))
                                    [pos] Y2 = E(Y + pos)
    swin_mlp   csrc/swin_mlp.hip    n = E(LN(x))   h = E(gelu(W1 n + b1))   y = E(W2 h + b2)   Y = E(y + x)

E rounds to the storage type (fp16 / bf16), and stands exactly where the kernels round (ffn_fused.hip:247, :263, :293 / :324,
:424, :494, :517, :548, :566; swin_mlp.hip:176, :237, :328).  The biases enter the fp32 accumulators (b1 as their initial
value, b2 / bo by one fp32 addition in front of the rounding); eps is the fp32 value the C entry receives.

`exact_ffn` / `exact_swin_mlp` evaluate this in float64 on the 16-bit inputs.  (E of a float64 goes through fp32: a value within
2^-29 of a rounding boundary can land on the other side of it.  The interval below straddles the boundary there, so the bound
covers either side; where the interval is empty -- the exact-integer cases -- every value is representable.)

`bound(exact)` is derived by carrying an interval [v - r, v + r] around every exact value v through the same stages:

    product    r' = |W| r + 2^-24 (K + 2) (|W| (|v| + r) + |bias|)    every fp32 addition of the K products and the bias, in any
                                                                       order (the products of two 16-bit values are exact in fp32)
    E          rounding is monotone: r' = max |E(v +- r) - E(v)|, which is 0 wherever the interval straddles no rounding boundary
    ReLU       monotone: r' = max |relu(v +- r) - relu(v)|
    sum        r' = ra + rb + 2^-24 (|v| + ra + rb)                    one fp32 addition (residual, pos)
    GELU       r' = 1.13 r + GELU_C (|v| + r)                          sup |gelu'| = 1.129; tests/epilogue_exact.py's measured bound
                                                                       of the kernels' gelu_erf
    LayerNorm  r' = fp32 (1 + rel) + |gamma| ((r + mean r) rstd (1 + rel) + |xhat| rel)
               fp32 = norm_bounds.bound_layernorm(.., n_s = C / 4 + 2).fp32: the kernels sum C / 4 in-lane values and two
               shuffles; rel = (1 - dv / (var + eps))^-1/2 - 1 for the change dv <= 2 mean(|x - mu| d) + mean(d^2), d = r + mean r,
               of the variance under a perturbation of the row by at most r

`emulate_*` repeat the kernels' rounding points in fp32 torch (any summation order) and take `mutant=`, one of FFN_MUTANTS /
SWIN_MUTANTS: the errors the cases below exist to catch.  `ffn_plan` / `swin_plan` restate the launchers' arithmetic
(ffn_fused.hip:620-647, swin_mlp.hip:346-352).

Two criteria hold a run (`measure`): every element within the bound, and the share of elements that differ from the exact value
at most 4 x the share of the emulation on the same inputs (pooled over the row counts of a case: a one-row call has 256
elements).  The second sees a biased rounding where hidden = 2048 drowns it in the worst-case accumulation radius.  It also
carries the oproj form: an interval widens at every product (|W| r takes every input at its worst at once) and every norm
spreads it over the row, so behind three products and two norms the bound is 20 - 300 x the error in fp16 and promises nothing
(inf: the interval of a row's variance reaches -eps) for most rows in bf16.  The plain form's bound is tight: an error of
exactly the bound, one step of the storage type where the interval straddles one rounding boundary, is the usual worst case.

Inputs are drawn from a CPU generator (the same values on every machine) and moved to `device`; the row counts come from the
device's CU count.
"""
import collections
import math

import torch

import epilogue_exact as ee
import norm_bounds as nb

E32 = nb.E32
GELU_LIP = 1.13
SHARE_FACTOR = 4.0
SHARE_MIN_COUNT = 8

FFN_MUTANTS = ("hidden_truncated", "hidden_kept_fp32", "y_not_rounded_before_residual", "w2_unpacked", "oproj_w1_unpermuted",
               "stale_ring_stage", "last_chunk_dropped", "ln_in_reads_ln_params", "one_pass_variance",
               "identity_is_raw_x_under_ln_in", "pos_added_before_ln", "second_launch_ignores_row_offset")
SWIN_MUTANTS = ("hidden_truncated", "hidden_kept_fp32", "y_not_rounded_before_residual", "w2_unpacked", "stale_ring_stage",
                "last_chunk_dropped", "one_pass_variance", "swin_residual_is_normed_x")

# form -> the optional stages of ffn_fused.hip that run
FORMS = {"plain": (), "plain_pos": ("pos",), "ln_in": ("ln_in",), "ln": ("ln",), "full": ("ln_in", "ln", "pos"),
         "oproj": ("oproj", "ln_in", "ln", "pos"), "oproj_plain": ("oproj", "pos")}
INT_LIMIT = {torch.float16: 2048, torch.bfloat16: 256}      # every integer up to here is a value of the type

Exact = collections.namedtuple("Exact", "out out2 stages inp")
Bound = collections.namedtuple("Bound", "out out2")
Launch = collections.namedtuple("Launch", "form row0 rows ntiles blocks walk")       # form: rows per workgroup, 128 or 64
Plan = collections.namedtuple("Plan", "launches nchunks walk")
Case = collections.namedtuple("Case", "name build Ms hidden form forms walk")
Result = collections.namedtuple("Result", "ratio share emu_ratio emu_share n")


# ------------------------------------------------------------------------------------------------------- plans
def ffn_plan(M, hidden, cus):
    """ffn_entry: 128-row tiles on one workgroup per CU; a left-over round of at most half the CUs goes to a second launch of the
    64-row form at a row offset"""
    T = -(-M // 128)
    left = T % cus
    split = left > 0 and 2 * left <= cus
    M1 = (T - left) * 128 if split else M
    launches = []
    for form, row0, rows in ((128, 0, M1), (64, M1, M - M1 if split else 0)):
        if rows > 0:
            nt = -(-rows // form)
            blocks = min(nt, cus)
            launches.append(Launch(form, row0, rows, nt, blocks, -(-nt // blocks)))
    return Plan(tuple(launches), hidden // 64, max(l.walk for l in launches))


def swin_plan(M, C, cus):
    """launch_swin_mlp: 128-row tiles; C = 192 runs two workgroups per CU on 32-wide hidden chunks, C = 384 one"""
    nt = -(-M // 128)
    blocks = min(nt, cus * (2 if C == 192 else 1))
    walk = -(-nt // blocks)
    return Plan((Launch(128, 0, M, nt, blocks, walk),), 4 * C // 32, walk)


def _walked_rows(plan, M, device):
    """[M] bool: the rows of a tile that is not the first of its workgroup"""
    m = torch.zeros(M, dtype=torch.bool, device=device)
    for l in plan.launches:
        m[l.row0 + l.blocks * l.form:l.row0 + l.rows] = True
    return m


def pack_w2_index(hidden):
    """pack_w2_kernel: packed column 32 s + 8 g + j of a 64-block takes column 32 s + 4 g + j (j < 4) | 32 s + 16 + 4 g + j - 4"""
    col = torch.arange(hidden)
    s, g, j = (col >> 5) & 1, (col >> 3) & 3, col & 7
    return (col & ~63) + 32 * s + torch.where(j < 4, 4 * g + j, 16 + 4 * g + j - 4)


def oproj_w1_index():
    """codetr_ffn_oproj_w1_index: column 32 s + 8 g + e of the permuted W1 takes column 32 s + 16 (g & 1) + 8 (g >> 1) + e"""
    col = torch.arange(256)
    s, g, e = col >> 5, (col >> 3) & 3, col & 7
    return 32 * s + 16 * (g & 1) + 8 * (g >> 1) + e


# ------------------------------------------------------------------------------------------------------- float64 and intervals
def _E(v, dt):
    return v.to(dt).double()


def _rnd(pre, r, dt):
    v = _E(pre, dt)
    if r is None:
        return v, None
    return v, torch.maximum((_E(pre + r, dt) - v).abs(), (_E(pre - r, dt) - v).abs())


def _prod(a, ra, w, bias, track):
    K = w.shape[1]
    pre = a @ w.t() + bias
    if not track:
        return pre, None
    wa = w.abs().t()
    if torch.is_tensor(ra):
        return pre, ra @ wa + E32 * (K + 2) * ((a.abs() + ra) @ wa + bias.abs())
    return pre, E32 * (K + 2) * (a.abs() @ wa + bias.abs())


def _add(a, ra, b, rb, track):
    pre = a + b
    return pre, (ra + rb + E32 * (pre.abs() + ra + rb)) if track else None


def _relu(v, r):
    o = v.clamp_min(0.0)
    if r is None:
        return o, None
    return o, torch.maximum((v + r).clamp_min(0.0) - o, o - (v - r).clamp_min(0.0))


def _gelu(v, r):
    o = 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))
    return o, None if r is None else GELU_LIP * r + ee.GELU_C * (v.abs() + r)


def _norm(v, r, ln, dt, track):
    g, b, eps = ln
    ex = nb.exact_layernorm(v.to(dt), g, b, eps)
    if not track:
        return ex.out, None
    n_s = v.shape[-1] // 4 + 2
    fp32 = nb.bound_layernorm(ex, n_s).fp32
    if not torch.is_tensor(r):
        return ex.out, fp32
    d = r + r.mean(-1, keepdim=True)
    dv = 2 * ((ex.x - ex.mu).abs() * d).mean(-1, keepdim=True) + (d * d).mean(-1, keepdim=True)
    rel = nb._rsqrt_rel(dv / (ex.var + ex.eps))
    lost = torch.isinf(rel)                       # the interval of the variance reaches -eps: nothing is promised for the row
    rel = rel.masked_fill(lost, 0.0)
    sens = ex.gamma.abs() * (d * ex.rstd * (1 + rel) + ex.xhat.abs() * rel)
    return ex.out, (fp32 * (1 + rel) + sens * (1 + E32 * (n_s + 7))).masked_fill(lost.expand_as(sens), math.inf)


def _walk_ffn(inp, track):
    dt, D, st = inp["dtype"], (lambda t: t.double()), []
    zero = 0.0 if track else None
    if "wo" in inp:
        v, r = _rnd(*_prod(D(inp["x"]), zero, D(inp["wo"]), D(inp["bo"]), track), dt)
        st.append(("oproj", v))
        v, r = _rnd(*_add(v, r, D(inp["ident"]), zero, track), dt)
        st.append(("x0", v))
    else:
        v, r = D(inp["x"]), zero
    if "ln_in" in inp:
        v, r = _rnd(*_norm(v, r, inp["ln_in"], dt, track), dt)
        st.append(("x1", v))
    x1, rx1 = v, r
    v, r = _relu(*_rnd(*_prod(x1, rx1, D(inp["w1"]), D(inp["b1"]), track), dt))
    st.append(("h", v))
    v, r = _rnd(*_prod(v, r, D(inp["w2"]), D(inp["b2"]), track), dt)
    st.append(("y", v))
    v, r = _rnd(*_add(v, r, x1, rx1, track), dt)
    st.append(("t", v))
    if "ln" in inp:
        v, r = _rnd(*_norm(v, r, inp["ln"], dt, track), dt)
    st.append(("Y", v))
    v2 = r2 = None
    if "pos" in inp:
        v2, r2 = _rnd(*_add(v, r, D(inp["pos"]), zero, track), dt)
        st.append(("Y2", v2))
    return v, r, v2, r2, st


def _walk_swin(inp, track):
    dt, D, st = inp["dtype"], (lambda t: t.double()), []
    x = D(inp["x"])
    v, r = _rnd(*_norm(x, 0.0 if track else None, inp["ln"], dt, track), dt)
    st.append(("n", v))
    v, r = _rnd(*_gelu(*_prod(v, r, D(inp["w1"]), D(inp["b1"]), track)), dt)
    st.append(("h", v))
    v, r = _rnd(*_prod(v, r, D(inp["w2"]), D(inp["b2"]), track), dt)
    st.append(("y", v))
    v, r = _rnd(*_add(v, r, x, 0.0 if track else None, track), dt)
    st.append(("Y", v))
    return v, r, None, None, st


def _walk(inp, track):
    return (_walk_swin if inp["kind"] == "swin" else _walk_ffn)(inp, track)


def exact_ffn(inp):
    """-> Exact(out, out2 | None, stages [(name, float64 value)], inp)"""
    assert inp["kind"] == "ffn"
    v, _, v2, _, st = _walk(inp, False)
    return Exact(v, v2, st, inp)


def exact_swin_mlp(inp):
    assert inp["kind"] == "swin"
    v, _, _, _, st = _walk(inp, False)
    return Exact(v, None, st, inp)


def exact(inp):
    return exact_swin_mlp(inp) if inp["kind"] == "swin" else exact_ffn(inp)


def bound(ex):
    """Bound(out, out2 | None): the derived elementwise bounds on |kernel - exact|"""
    _, r, _, r2, _ = _walk(ex.inp, True)
    wide = lambda t: None if t is None else t.nan_to_num(nan=math.inf, posinf=math.inf)   # noqa: E731  (inf - inf, 0 inf)
    return Bound(wide(r), wide(r2))


def ratio(got, want, tol):
    """largest |got - want| / tol; inf where an element lies outside (a non-finite output included)"""
    err = (got.double() - want).abs()
    if not bool((err <= tol).all()) or not bool(torch.isfinite(got).all()):
        return math.inf
    return (err / tol.clamp_min(1e-300)).max().item()


def differing(got, want):
    """the number of elements that are not the exact value"""
    return int((got.double() != want).sum())


# ------------------------------------------------------------------------------------------------------- emulations
def _ln32(x, ln, one_pass):
    g, b, eps = ln
    eps = torch.tensor(eps, dtype=torch.float32, device=x.device)
    mean = x.mean(-1, keepdim=True)
    if one_pass:
        var = (x * x).mean(-1, keepdim=True) - mean * mean
    else:
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * g.float() + b.float()


def _mlp32(xin, inp, act, chunk, mutant, walked):
    """(W2 act(E(W1 xin + b1)) + b2 in fp32, before its rounding) with the hidden-side mutants"""
    dt = inp["dtype"]
    w1, b1, w2 = inp["w1"].float(), inp["b1"].float(), inp["w2"].float()

    def run(w1, w2):
        z = xin @ w1.t() + b1
        if act == "gelu":
            z = ee.gelu_emulated(z)
        if mutant == "hidden_truncated":
            h = ee.round_trunc(z, dt).float()
        elif mutant == "hidden_kept_fp32":
            h = z
        else:
            h = z.to(dt).float()
        if act == "relu":
            h = h.clamp_min(0.0)
        if mutant == "last_chunk_dropped":
            h = torch.cat([h[:, :-chunk], torch.zeros_like(h[:, -chunk:])], 1)
        if mutant == "w2_unpacked":
            h = h[:, pack_w2_index(h.shape[1]).to(h.device)]
        return h @ w2.t()

    y = run(w1, w2)
    if mutant == "stale_ring_stage" and bool(walked.any()):
        # chunk 0 of a later tile reads the stage the previous tile's last chunk left (b1 comes from its own table)
        stale = run(torch.cat([w1[-chunk:], w1[chunk:]], 0), torch.cat([w2[:, -chunk:], w2[:, chunk:]], 1))
        y = torch.where(walked[:, None], stale, y)
    return y + inp["b2"].float()


def emulate_ffn(inp, mutant=None, cus=256):
    """-> (Y, Y2 | None) in the storage type; rows of Y2 that a mutant leaves unwritten are zero"""
    assert inp["kind"] == "ffn" and (mutant is None or mutant in FFN_MUTANTS)
    dt, M = inp["dtype"], inp["x"].shape[0]
    R = lambda t: t.to(dt).float()   # noqa: E731
    plan = ffn_plan(M, inp["w1"].shape[0], cus)
    second = next((l for l in plan.launches if l.form == 64 and l.row0 > 0), None)

    def offset_lost(t):              # what the 64-row launch reads when it takes its rows from the start of the tensor
        if mutant != "second_launch_ignores_row_offset" or second is None:
            return t
        return torch.cat([t[:second.row0], t[:second.rows]], 0)

    one_pass = mutant == "one_pass_variance"
    x = inp["x"].float()
    if "wo" in inp:
        x = R(R(x @ inp["wo"].float().t() + inp["bo"].float()) + offset_lost(inp["ident"]).float())
    x1 = x
    if "ln_in" in inp:
        x1 = R(_ln32(x, inp["ln"] if mutant == "ln_in_reads_ln_params" and "ln" in inp else inp["ln_in"], one_pass))
    xin = x1
    if mutant == "oproj_w1_unpermuted" and "wo" in inp:
        xin = x1[:, oproj_w1_index().to(x1.device)]
    y = _mlp32(xin, inp, "relu", 64, mutant, _walked_rows(plan, M, x.device))
    resid = x if mutant == "identity_is_raw_x_under_ln_in" and "ln_in" in inp else x1
    t = R(y + resid) if mutant == "y_not_rounded_before_residual" else R(R(y) + resid)
    Y = R(_ln32(t, inp["ln"], one_pass)) if "ln" in inp else t
    if "pos" not in inp:
        return Y.to(dt), None
    pos = offset_lost(inp["pos"]).float()
    if mutant == "pos_added_before_ln" and "ln" in inp:
        Y2 = R(_ln32(R(t + pos), inp["ln"], one_pass))
    else:
        Y2 = R(Y + pos)
    if mutant == "second_launch_ignores_row_offset" and second is not None:
        Y2 = torch.cat([Y2[second.row0:], Y2[second.rows:second.row0], torch.zeros_like(Y2[second.row0:])], 0)
    return Y.to(dt), Y2.to(dt)


def emulate_swin_mlp(inp, mutant=None, cus=256):
    assert inp["kind"] == "swin" and (mutant is None or mutant in SWIN_MUTANTS)
    dt, (M, C) = inp["dtype"], inp["x"].shape
    R = lambda t: t.to(dt).float()   # noqa: E731
    x = inp["x"].float()
    n = R(_ln32(x, inp["ln"], mutant == "one_pass_variance"))
    y = _mlp32(n, inp, "gelu", 32, mutant, _walked_rows(swin_plan(M, C, cus), M, x.device))
    resid = n if mutant == "swin_residual_is_normed_x" else x
    Y = R(y + resid) if mutant == "y_not_rounded_before_residual" else R(R(y) + resid)
    return Y.to(dt), None


def emulate(inp, mutant=None, cus=256):
    return (emulate_swin_mlp if inp["kind"] == "swin" else emulate_ffn)(inp, mutant, cus)


# ------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def to_device(inp, device):
    mv = lambda v: v.to(device) if torch.is_tensor(v) else v   # noqa: E731
    return {k: tuple(mv(e) for e in v) if isinstance(v, tuple) else mv(v) for k, v in inp.items()}


def _affine(dt, g, eps, scale=1.0, C=256):
    return (scale * (1 + 0.1 * torch.randn(C, generator=g))).to(dt), (scale * 0.1 * torch.randn(C, generator=g)).to(dt), eps


def ffn_random(M, hidden, dt, form="plain", seed=0):
    """the scales of the model's encoder FFN; different parameters and eps for the two norms; every row of pos / identity its own"""
    g, fl = _gen(1000 * seed + M + hidden), FORMS[form]
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dt)   # noqa: E731
    inp = dict(kind="ffn", dtype=dt, x=r(M, 256), w1=r(hidden, 256, k=1 / 16), b1=r(hidden, k=0.5),
               w2=r(256, hidden, k=hidden ** -0.5), b2=r(256, k=0.5))
    if "oproj" in fl:
        inp.update(wo=r(256, 256, k=1 / 16), bo=r(256, k=0.5), ident=r(M, 256, k=2.0))
    if "ln_in" in fl:
        inp["ln_in"] = _affine(dt, g, 1e-4)
    if "ln" in fl:
        inp["ln"] = _affine(dt, g, 1e-5)
    if "pos" in fl:
        inp["pos"] = r(M, 256)
    return inp


def ffn_distinct(M, hidden, dt, form="full", seed=0):
    """rows of variance 1e-4 .. 1e-3 under ln_in_eps = 1e-3 and ln_eps = 1e-5, small gamma_in and W2 so that the second norm sees
    such rows too; row 0 is a constant (form ln_in: x1 = beta_in bit for bit), row 1 is 0 under b1 <= 0 and a constant b2 (form
    ln: h = 0, t = b2, Y = beta bit for bit), rows 2 .. 9 are 100 +- 0.05 (constants in bf16, whose step there is 0.5), rows
    10 .. 17 are 100 +- 0.5"""
    g, fl = _gen(77 + M + seed), FORMS[form]
    sigma = 10.0 ** (-2 + 0.5 * torch.rand(M, 1, generator=g))
    x = 0.25 * (2 * torch.rand(M, 1, generator=g) - 1) + sigma * torch.randn(M, 256, generator=g)
    x[0] = 0.375
    if M > 1:
        x[1] = 0.0
    if M >= 18:
        x[2:10] = 100.0 + 0.05 * torch.randn(8, 256, generator=g)
        x[10:18] = 100.0 + 0.5 * torch.randn(8, 256, generator=g)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k   # noqa: E731
    k_in = 0.03 if "ln_in" in fl else 1.0
    inp = dict(kind="ffn", dtype=dt, x=x.to(dt), w1=r(hidden, 256, k=1 / 16).to(dt), b1=(-r(hidden, k=0.02).abs()).to(dt),
               w2=r(256, hidden, k=0.05 * hidden ** -0.5).to(dt), b2=torch.full((256,), 0.25).to(dt))
    if "ln_in" in fl:
        inp["ln_in"] = _affine(dt, g, 1e-3, scale=k_in)
    if "ln" in fl:
        inp["ln"] = _affine(dt, g, 1e-5)
    if "pos" in fl:
        inp["pos"] = r(M, 256).to(dt)
    return inp


def _sparse_pm1(rows, cols, nnz, g):
    """[rows, cols] with nnz entries of +-1 per row"""
    w = torch.zeros(rows, cols)
    idx = torch.rand(rows, cols, generator=g).argsort(1)[:, :nnz]
    w.scatter_(1, idx, (2.0 * torch.randint(0, 2, (rows, nnz), generator=g) - 1))
    return w


def ffn_exact(M, hidden, dt, form="plain_pos", seed=0):
    """small integers, sparse +-1 weights: every intermediate is an integer of the storage type, so E never rounds and the
    float64 result is the only right answer.  Four +-1 per row of Wo and W1, three per row of W2:
    |x1| <= 4 2 + 2 + 3 = 13 (oproj) | 3;  |h| <= 4 |x1| + 2;  |y| <= 3 |h| + 2;  |Y2| <= |y| + |x1| + 3 <= 180"""
    g, fl = _gen(31 + M + hidden + seed), FORMS[form]
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()   # noqa: E731
    inp = dict(kind="ffn", dtype=dt, w1=_sparse_pm1(hidden, 256, 4, g), b1=ri(-2, 2, hidden), w2=_sparse_pm1(256, hidden, 3, g),
               b2=ri(-2, 2, 256), pos=ri(-3, 3, M, 256))
    if "oproj" in fl:
        inp.update(x=ri(-2, 2, M, 256), wo=_sparse_pm1(256, 256, 4, g), bo=ri(-2, 2, 256), ident=ri(-3, 3, M, 256))
    else:
        inp["x"] = ri(-3, 3, M, 256)
    return {k: v.to(dt) if torch.is_tensor(v) else v for k, v in inp.items()}


# (row period, column period) of the routing values: the type holds R x Cm / 2 integers either side of zero, so one pattern
# resolves the row within a 16-row tile and the other every column
ROUTING = {torch.float16: ((16, 64), (4, 256)), torch.bfloat16: ((16, 16), (1, 256))}


def ffn_routing(M, dt, variant, form="plain_pos", seed=0):
    """W1, W2 (and Wo) one-hot, hidden = 512: h = (relu(x_p), relu(-x_p)), y_n = h_q(n) - h_256+q(n) = x_p(q(n)), Y = y + x; with
    x[m][c] = R (c mod Cm) + m mod R - R Cm / 2 a wrong lane, k-slot or swizzle shows as another row's or channel's integer"""
    g, fl = _gen(5 + variant + seed), FORMS[form]
    R, Cm = ROUTING[dt][variant]
    m, c = torch.arange(M)[:, None], torch.arange(256)[None]
    x = (R * (c % Cm) + m % R - R * Cm // 2).float()
    p, q = torch.randperm(256, generator=g), torch.randperm(256, generator=g)
    eye = torch.eye(256)
    w1 = torch.cat([eye[p], -eye[p]], 0)
    w2 = torch.cat([eye[q], -eye[q]], 1)
    inp = dict(kind="ffn", dtype=dt, x=x, w1=w1, b1=torch.zeros(512), w2=w2, b2=torch.zeros(256), pos=torch.zeros(M, 256))
    if "oproj" in fl:
        inp.update(wo=eye[torch.randperm(256, generator=g)], bo=torch.zeros(256), ident=torch.zeros(M, 256))
    return {k: v.to(dt) if torch.is_tensor(v) else v for k, v in inp.items()}


def ffn_coherent(M, hidden, dt, seed=0):
    """W2 > 0 and b2 = -mean of the branch: a hidden pack that rounds every value the same way moves y by hidden x half a step
    of h times W2, where unbiased roundings cancel to sqrt(hidden) of that"""
    inp = ffn_random(M, hidden, dt, "plain", seed + 9)
    g = _gen(seed + 10)
    w2 = ((0.5 + 0.5 * torch.rand(256, hidden, generator=g)) * hidden ** -0.5).to(dt)
    h = torch.relu(inp["x"].double() @ inp["w1"].double().t() + inp["b1"].double())
    inp.update(w2=w2, b2=(-(h @ w2.double().t()).mean(0)).to(dt))
    return inp


def swin_random(M, C, dt, seed=0):
    """the scales of tests/test_swin_mlp_gpu.py: rows with a common offset per channel and an offset of their own"""
    g = _gen(1000 * seed + M + C)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k   # noqa: E731
    x = r(M, C, k=1.5) + r(1, C, k=0.5) + r(M, 1, k=0.5)
    return dict(kind="swin", dtype=dt, x=x.to(dt), ln=((1.0 + 0.2 * r(C)).to(dt), r(C, k=0.2).to(dt), 1e-5),
                w1=r(4 * C, C, k=C ** -0.5).to(dt), b1=r(4 * C, k=0.3).to(dt), w2=r(C, 4 * C, k=(4 * C) ** -0.5).to(dt),
                b2=r(C, k=0.3).to(dt))


def swin_offset(M, C, dt, seed=0):
    """rows at 100 +- 0.25: a variance taken as mean(x^2) - mean^2 in fp32 is off by a few 1e-2 of it"""
    inp = swin_random(M, C, dt, seed + 3)
    inp["x"] = (100.0 + 0.25 * torch.randn(M, C, generator=_gen(seed + 4))).to(dt)
    return inp


def swin_coherent(M, C, dt, seed=0):
    inp = swin_random(M, C, dt, seed + 9)
    g = _gen(seed + 10)
    w2 = ((0.5 + 0.5 * torch.rand(C, 4 * C, generator=g)) * (4 * C) ** -0.5).to(dt)
    n = nb.exact_layernorm(inp["x"], *inp["ln"]).out.to(dt).double()
    h = torch.nn.functional.gelu(n @ inp["w1"].double().t() + inp["b1"].double())
    inp.update(w2=w2, b2=(-(h @ w2.double().t()).mean(0)).to(dt))
    return inp


# ------------------------------------------------------------------------------------------------------- cases
TAIL_M = (1, 15, 17, 63, 64, 65, 129)
SWIN_TAIL_M = (1, 31, 33, 127, 129)


def ragged_M(cus):
    """the 128-row form alone; the last tile ends inside wave 2, wave 3 is all clamped rows"""
    return 128 * (cus // 2) + 77


def multi_M(cus):
    """the 128-row form alone, cus / 2 + 1 workgroups walk a second tile"""
    return 128 * (cus + cus // 2 + 1) - 50


def split_M(cus):
    """one full round of the 128-row form, then 197 rows (64 + 64 + 64 + 5) of the 64-row form at row offset 128 cus"""
    return 128 * cus + 197


def swin_walk_M(C, cus):
    return 128 * (cus * (2 if C == 192 else 1) + 1) + 45


def ffn_cases(cus):
    """name -> Case: the builder, the row counts (pooled), hidden, the form, and what the plan must say: which launch forms run
    and how many tiles the busiest workgroup walks"""
    cs = []
    for hidden in (64, 2048):
        for form in ("plain", "full"):
            cs.append(Case(f"tails_h{hidden}_{form}", "random", TAIL_M, hidden, form, (64,), 1))
    for form in ("plain", "full"):
        cs.append(Case(f"ragged_{form}", "random", (ragged_M(cus),), 2048, form, (128,), 1))
    for hidden in (64, 128, 192):
        for form in ("plain", "oproj"):
            cs.append(Case(f"multi_h{hidden}_{form}", "random", (multi_M(cus),), hidden, form, (128,), 2))
    for form in ("full", "oproj"):
        cs.append(Case(f"split_{form}", "random", (split_M(cus),), 2048, form, (128, 64), 1))
    cs.append(Case("distinct_small", "distinct", (200,), 256, "full", (64,), 1))
    cs.append(Case("distinct_ragged", "distinct", (ragged_M(cus),), 256, "full", (128,), 1))
    for form in ("plain_pos", "oproj_plain"):
        cs.append(Case(f"exact_tails_{form}", "exact", TAIL_M, 192, form, (64,), 1))
        cs.append(Case(f"exact_split_{form}", "exact", (split_M(cus),), 192, form, (128, 64), 1))
        for v in (0, 1):
            cs.append(Case(f"routing{v}_tails_{form}", f"routing{v}", TAIL_M, 512, form, (64,), 1))
            cs.append(Case(f"routing{v}_split_{form}", f"routing{v}", (split_M(cus),), 512, form, (128, 64), 1))
    for hidden in (64, 512):
        cs.append(Case(f"coherent_h{hidden}", "coherent", (200,), hidden, "plain", (64,), 1))
    return {c.name: c for c in cs}


def swin_cases(cus):
    cs = []
    for C in (192, 384):
        cs.append(Case(f"tails_c{C}", "random", SWIN_TAIL_M, 4 * C, C, (128,), 1))
        cs.append(Case(f"walk_c{C}", "random", (swin_walk_M(C, cus),), 4 * C, C, (128,), 2))
        cs.append(Case(f"coherent_c{C}", "coherent", (200,), 4 * C, C, (128,), 1))
        cs.append(Case(f"offset_c{C}", "offset", (200,), 4 * C, C, (128,), 1))
    return {c.name: c for c in cs}


FFN_CASE_NAMES = tuple(ffn_cases(4))
SWIN_CASE_NAMES = tuple(swin_cases(4))


def build(case, M, dt):
    """the inputs of one row count of a case, on the CPU"""
    if isinstance(case.form, int):
        return {"coherent": swin_coherent, "offset": swin_offset, "random": swin_random}[case.build](M, case.form, dt)
    if case.build == "random":
        return ffn_random(M, case.hidden, dt, case.form)
    if case.build == "distinct":
        return ffn_distinct(M, case.hidden, dt, case.form)
    if case.build == "exact":
        return ffn_exact(M, case.hidden, dt, case.form)
    if case.build == "coherent":
        return ffn_coherent(M, case.hidden, dt)
    return ffn_routing(M, dt, int(case.build[-1]), case.form)


def measure(case, dt, run, device="cpu", cus=256, emulated=True):
    """run(inp) -> (Y, Y2 | None) over every row count of the case -> Result: the largest err / bound (inf where an element lies
    outside) and the share of elements that differ from the exact value, for `run` and for the emulation on the same inputs"""
    worst, diff, e_worst, e_diff, n = 0.0, 0, 0.0, 0, 0
    for M in case.Ms:
        inp = to_device(build(case, M, dt), device)
        ex = exact(inp)
        b = bound(ex)
        runs = [run(inp)] + ([emulate(inp, None, cus)] if emulated else [])
        for k, (y, y2) in enumerate(runs):
            assert y.dtype == dt and y.shape == ex.out.shape and (y2 is None) == (ex.out2 is None)
            w, d = ratio(y, ex.out, b.out), differing(y, ex.out)
            if y2 is not None:
                w, d = max(w, ratio(y2, ex.out2, b.out2)), d + differing(y2, ex.out2)
            if k == 0:
                worst, diff = max(worst, w), diff + d
            else:
                e_worst, e_diff = max(e_worst, w), e_diff + d
        n += ex.out.numel() * (1 if ex.out2 is None else 2)
    return Result(worst, diff / n, e_worst, e_diff / n, n)


def share_cap(res):
    """4 x the emulation's share: the kernel's summation order is not the emulation's, and shares of this kind move by small
    factors.  Both are counts of rare independent events, so a count below SHARE_MIN_COUNT is its own noise (sigma = sqrt(count),
    and an emulation that happens to flip nothing says little about the next summation order): it counts as SHARE_MIN_COUNT"""
    return SHARE_FACTOR * max(res.emu_share, SHARE_MIN_COUNT / res.n)


def holds(res):
    """the two criteria (err == bound is inside: both are distances between neighbouring values of the storage type)"""
    return res.ratio <= 1.0 and res.share <= share_cap(res)
