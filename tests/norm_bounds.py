"""float64 references, derived error bounds, CPU emulations and test inputs for the normalisation kernels (pure torch: the same
code runs on the CPU and on the device; tests/test_norm_bounds_cpu.py proves the bounds and the cases,
tests/test_layernorm_gpu.py and tests/test_groupnorm_gpu.py run the kernels).

    layernorm   csrc/layernorm.hip          y = (x - mean) rsqrt(var + eps) gamma + beta over the last axis, two-pass
    merge       csrc/layernorm.hip (MERGE)  the same over the 2 x 2 gather of a token map, (ky, kx, c) order, zeros beyond an odd H / W
    groupnorm   csrc/groupnorm_tokens.hip   statistics over HW x 8 per (image, group): fp32 partials, taken again about
                                            the first mean where they lost the variance

`exact_*` evaluate the formula in float64 on the 16-bit inputs (eps as the fp32 value the C entry receives) and return an
`Exact`: out, mu, var, rstd, xhat, and the float64 x / gamma / beta they were computed from.

`bound_*(exact)` -- where the kernels round.  u = storage unit roundoff (fp16 2^-11, bf16 2^-8), e = 2^-24 (fp32).  With an
absolute error e_mean of the kernel's mean and a relative error rel of its rstd, both kernels end in
(layernorm.hip:128, groupnorm_tokens.hip:163)

    y = store(fmaf((x - mean) * rstd, gamma, beta))
    fp32  = |gamma| X (1 + e) + e |y|,   X = (|xhat| (rel + 2 e) + e_mean rstd) (1 + rel)     subtraction, product, fmaf
    total = u (|y| + fp32) + tiny + fp32                       the store; tiny = half a step below the normal range of the
                                                               storage type: fp16 2^-25, bf16 2^-126

LayerNorm, G lanes x NCH chunks of 8 (`ln_config`, layernorm.hip:168-179); n_s = 8 NCH + log2 G additions lie between an
element and the row sum (the lane's chain :103 / :115, the butterfly :46):

    e_mean = e (n_s + 2) mean|x|                  the chain, the product with 1/C and the rounding of 1.0f / C itself (:67, :106)
    e_var  = e (n_s + 5) (var + e_mean^2 + eps) + e_mean^2
                                                  d = x - mean rounded once, so d^2 twice (:114); the fmaf chain and butterfly;
                                                  1/C and the product; the + eps (:119).  The deviations are taken from the
                                                  kernel's own mean: sum (x - mu) = 0 removes the cross term and leaves e_mean^2
    rel    = (1 - e_var / (var + eps))^-1/2 - 1 + 2 e          rsqrtf is good to one ulp = 2 e (:119)

GroupNorm, rows_par = 256 / groups rows in parallel, R = ceil(128 / rows_par) rows per lane and slab.  Sums of x - K and
(x - K)^2 that lie n_s additions deep in arithmetic of unit roundoff e', reduced in fp64 (`bound_groupnorm_sums`), with
d = x - K, m' = mu - K:

    e_s    = e' (n_s + 1) mean|d|                 d rounded once
    e_mean = e_s + e |mu|                         mean = (float)(K + s / n) (groupnorm_tokens.hip:140)
    e_var  = e' (n_s + 2) (var + m'^2) + 2 |m'| e_s + e_s^2     q / n - (s / n)^2: sum d^2 / n = var + m'^2
    rel    = (1 - e_var / (var + eps))^-1/2 - 1 + e            rstd cast to float (:141)

so the variance term is e' (n_s + 2) (1 + rho') + ... relative to var, rho' = m'^2 / var.  The kernel (`bound_groupnorm`) takes
fp32 partials of x and x^2 (K = 0, e' = e, n_s = 8 R + rows_par: the lane's chain :80-81, the LDS adds :92-93), forms from them
the very bound above with mean|x| <= sqrt(q / n) (`gn_lost`, :135-136) and, where that exceeds thresh (var + eps) -- thresh =
2^-13 for fp16, 2^-10 for bf16: an eighth of u -- takes the same sums again about K = (float) of that first mean (:137-138,
:69-71), so |m'| <= the first e_mean.  A bound of inf (e_var >= var + eps) says that a contract promises nothing there:
resum=False, the fp32 partials alone, at 100 +- 0.05.

`emulate_*` repeat the kernels' rounding points in fp32 torch (lane order, butterfly, fmaf as a float64 product rounded once,
multiplication by the rounded 1/C) and take `mutant=`, one of LN_MUTANTS / MERGE_MUTANTS / GN_MUTANTS: the errors the cases
below exist to catch.  They are not bit-exact.

Inputs are drawn from a CPU generator (the same values on every machine) and moved to `device`.
"""
import collections
import math

import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -126}
E32 = 2.0 ** -24
E64 = 2.0 ** -53
# gn_finalize_kernel flags a group for the pivoted sums where the partials may have lost more than this of var + eps
GN_RESUM = {torch.float16: 2.0 ** -13, torch.bfloat16: 2.0 ** -10}
SLAB = 128                     # rows per workgroup of gn_partial_kernel
GN_THREADS = 256

LN_MUTANTS = ("one_pass_variance", "unbiased_variance", "eps_outside_sqrt", "stats_skip_last_chunk",
              "stats_over_32_lanes_when_64", "affine_chunk_shifted", "normalised_rounded_before_affine")
MERGE_MUTANTS = ("swap_ky_kx", "pad_clamps_instead_of_zero", "row_decode_uses_W_not_W2")
GN_MUTANTS = ("fp32_sums_no_pivot", "last_slab_dropped", "count_uses_full_slabs", "stats_of_previous_image",
              "group_spans_16_channels", "eps_outside_sqrt", "dest_ignores_batch_stride")

Exact = collections.namedtuple("Exact", "out mu var rstd xhat x gamma beta eps dtype")
Bound = collections.namedtuple("Bound", "total fp32")


def eps_f32(eps):
    """the eps the C entry receives: a float"""
    return torch.tensor(eps, dtype=torch.float32).item()


# ------------------------------------------------------------------------------------------------------- float64
def exact_layernorm(x, gamma, beta, eps):
    """x [..., C], gamma, beta [C] 16-bit -> Exact; mu, var, rstd are [..., 1]"""
    xd, g, b, eps = x.double(), gamma.double(), beta.double(), eps_f32(eps)
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xhat = (xd - mu) * rstd
    return Exact(xhat * g + b, mu, var, rstd, xhat, xd, g, b, eps, x.dtype)


def exact_patch_merge(x4d):
    """[B, H, W, Cs] -> [B, H2 W2, 4 Cs]: pad to even sizes with zeros, 2 x 2 blocks, (ky, kx, c) order (by views, not indices)"""
    B, H, W, Cs = x4d.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    x4 = torch.nn.functional.pad(x4d, (0, 0, 0, W % 2, 0, H % 2))
    return x4.view(B, H2, 2, W2, 2, Cs).permute(0, 1, 3, 2, 4, 5).reshape(B, H2 * W2, 4 * Cs)


def exact_patch_merge_layernorm(x4d, gamma, beta, eps):
    return exact_layernorm(exact_patch_merge(x4d), gamma, beta, eps)


def exact_groupnorm_tokens(x, gamma, beta, groups, eps):
    """x [B, HW, C = 8 groups] -> Exact with out, xhat, x [B, HW, groups, 8]; mu, var, rstd [B, 1, groups, 1]"""
    B, HW, C = x.shape
    assert C == groups * 8
    xd, eps = x.double().view(B, HW, groups, 8), eps_f32(eps)
    g, b = gamma.double().view(groups, 8), beta.double().view(groups, 8)
    mu = xd.mean((1, 3), keepdim=True)
    var = ((xd - mu) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + eps) ** -0.5
    xhat = (xd - mu) * rstd
    return Exact(xhat * g + b, mu, var, rstd, xhat, xd, g, b, eps, x.dtype)


# ------------------------------------------------------------------------------------------------------- bounds
def ln_config(C):
    """(G lanes per row, NCH chunks per lane) of `launch` (layernorm.hip:168-179)"""
    nch = C // 8
    for limit, cfg in ((32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (192, (64, 3)), (256, (64, 4)), (384, (64, 6))):
        if nch <= limit:
            return cfg
    return 64, 8


def gn_depth(groups):
    """additions between a value and its slab sum in gn_partial_kernel: the lane's chain through 8 x R values, then the LDS adds"""
    rows_par = GN_THREADS // groups
    R = -(-SLAB // rows_par)
    return 8 * R + rows_par


def _rsqrt_rel(t):
    """relative error of (v + eps)^-1/2 for a relative error t of v + eps; inf where t >= 1"""
    return torch.where(t < 1, (1 - t).clamp_min(1e-300) ** -0.5 - 1, torch.full_like(t, math.inf))


def _assemble(ex, rel, e_mean):
    u, g = U[ex.dtype], ex.gamma.abs()
    X = (ex.xhat.abs() * (rel + 2 * E32) + e_mean * ex.rstd) * (1 + rel)
    fp32 = g * X * (1 + E32) + E32 * ex.out.abs()
    return Bound(u * (ex.out.abs() + fp32) + TINY[ex.dtype] + fp32, fp32)


def bound_layernorm(ex, n_s=None):
    """Bound(total, fp32): the derived elementwise bound on |kernel - ex.out| and the part of it that fp32 arithmetic owns.
    n_s: the additions between an element and the row sum, for a kernel that sums in another shape than layernorm.hip's
    (the fused FFN / Swin MLP epilogues: C / 4 in-lane values and two shuffles, tests/ffn_bounds.py)"""
    if n_s is None:
        G, NCH = ln_config(ex.out.shape[-1])
        n_s = 8 * NCH + int(math.log2(G))
    e_mean = E32 * (n_s + 2) * ex.x.abs().mean(-1, keepdim=True)
    e_var = E32 * (n_s + 5) * (ex.var + e_mean ** 2 + ex.eps) + e_mean ** 2
    rel = _rsqrt_rel(e_var / (ex.var + ex.eps)) + 2 * E32
    return _assemble(ex, rel, e_mean)


def _sums_bound(ex, mp, dabs, n_s, e=E32):
    """sums of x - K and (x - K)^2, n_s additions deep in arithmetic of unit roundoff e, reduced in fp64, for |mu - K| <= mp and
    mean|x - K| <= dabs"""
    e_s = e * (n_s + 1) * dabs
    e_mean = e_s + E32 * ex.mu.abs()
    e_var = e * (n_s + 2) * (ex.var + mp ** 2) + 2 * mp * e_s + e_s ** 2
    rel = _rsqrt_rel(e_var / (ex.var + ex.eps)) + E32
    return _assemble(ex, rel, e_mean), e_mean


def bound_groupnorm_sums(ex, K, n_s, e=E32):
    """the contract of sums about a given K ([B, 1, groups, 1] or a number)"""
    return _sums_bound(ex, (ex.mu - K).abs(), (ex.x - K).abs().mean((1, 3), keepdim=True), n_s, e)[0]


def gn_lost(ex):
    """the finalize kernel's own estimate of what the fp32 partials lost of var, over its threshold (groupnorm_tokens.hip:135-136),
    on the exact statistics: > 1 means that the group is flagged and summed again about the pivot"""
    n = gn_depth(ex.out.shape[2])
    e2 = ex.var + ex.mu ** 2
    lost = E32 * ((n + 2) * e2 + 2 * (n + 1) * ex.mu.abs() * e2.sqrt())
    return lost / (GN_RESUM[ex.dtype] * (ex.var + ex.eps))


def bound_groupnorm(ex, resum=True):
    """the kernel's contract: the fp32 partials where `gn_lost` <= 1; where it is > 1, the same sums about K = (float) mean of
    the first reduction, which lies within the partials' e_mean of mu; the larger of the two within 1e-3 of the threshold (the
    kernel decides on its own var, which is good to the threshold there).
    resum=False: the fp32 partials everywhere -- the kernel before it checked them"""
    n = gn_depth(ex.out.shape[2])
    mean_abs = ex.x.abs().mean((1, 3), keepdim=True)
    partials, e_mean = _sums_bound(ex, ex.mu.abs(), mean_abs, n)
    if not resum:
        return partials
    again, _ = _sums_bound(ex, e_mean, (ex.x - ex.mu).abs().mean((1, 3), keepdim=True) + e_mean, n)
    z = gn_lost(ex)
    pick = lambda p, a: torch.where(z < 0.999, p, torch.where(z > 1.001, a, torch.maximum(p, a)))
    return Bound(pick(partials.total, again.total), pick(partials.fp32, again.fp32))


def ratio(got, exact_out, tol):
    """largest |got - exact| / tol; a non-finite output counts as infinitely wrong"""
    err = (got.double().reshape(exact_out.shape) - exact_out).abs()
    if not torch.isfinite(err).all():
        return math.inf
    return (err / tol).max().item()


def fp32_share(ex, b):
    """largest fp32 part of the bound over u (|gamma| max(|xhat|, 1) + |beta|) / 4"""
    ref = U[ex.dtype] * (ex.gamma.abs() * ex.xhat.abs().clamp_min(1.0) + ex.beta.abs()) / 4
    return (b.fp32 / ref).max().item()


def dest_ratio(dest, row_start, HW, sentinel, ex, tol):
    """`ratio` of the destination slice dest[:, row_start : row_start + HW]; inf when a neighbouring row lost its sentinel"""
    if not ((dest[:, :row_start] == sentinel).all() and (dest[:, row_start + HW:] == sentinel).all()):
        return math.inf
    return ratio(dest[:, row_start:row_start + HW], ex.out, tol)


# ------------------------------------------------------------------------------------------------------- emulations
def _fma(a, b, c):
    """one fp32 rounding of a b + c"""
    return (a.double() * b.double() + c.double()).float()


def _butterfly(v, width):
    """v [rows, G]: the __shfl_xor sum over aligned groups of `width` lanes"""
    idx = torch.arange(v.shape[-1], device=v.device)
    o = width // 2
    while o > 0:
        v = v + v[:, idx ^ o]
        o //= 2
    return v


def emulate_layernorm(x, gamma, beta, eps, mutant=None):
    """x [..., C] 16-bit -> the same shape and type"""
    assert mutant is None or mutant in LN_MUTANTS
    dtype, f, shape = x.dtype, torch.float32, x.shape
    C = shape[-1]
    x = x.reshape(-1, C)
    rows = x.shape[0]
    G, NCH = ln_config(C)
    nchunks, P = C // 8, NCH * G * 8
    eps = torch.tensor(eps, dtype=f, device=x.device)

    def lanes(t, lead):
        """[lead.., C] -> [lead.., NCH, G, 8] zero-padded: chunk ch = sub + c G of lane sub"""
        p = torch.zeros(lead + (P,), dtype=f, device=x.device)
        p[..., :C] = t.float()
        return p.view(lead + (NCH, G, 8))

    xv, gv, bv = lanes(x, (rows,)), lanes(gamma, ()), lanes(beta, ())
    ch = torch.arange(NCH, device=x.device)[:, None] * G + torch.arange(G, device=x.device)[None]      # [NCH, G]
    counted = ch < (nchunks - 1 if mutant == "stats_skip_last_chunk" else nchunks)
    inv_c = torch.tensor(1.0, dtype=f, device=x.device) / torch.tensor(float(C), dtype=f, device=x.device)
    width = 32 if mutant == "stats_over_32_lanes_when_64" else G

    s = torch.zeros(rows, G, dtype=f, device=x.device)
    for c in range(NCH):
        for e in range(8):
            s = torch.where(counted[c], s + xv[:, c, :, e], s)
    mean = _butterfly(s, width) * inv_c                                                                 # [rows, G]
    q = torch.zeros(rows, G, dtype=f, device=x.device)
    for c in range(NCH):
        for e in range(8):
            d = xv[:, c, :, e] if mutant == "one_pass_variance" else xv[:, c, :, e] - mean
            q = torch.where(counted[c], _fma(d, d, q), q)
    q = _butterfly(q, width)
    if mutant == "unbiased_variance":
        var = q * (torch.tensor(1.0, dtype=f, device=x.device) / torch.tensor(float(max(C - 1, 1)), dtype=f, device=x.device))
    else:
        var = q * inv_c
    if mutant == "one_pass_variance":
        var = var - mean * mean
    rstd = 1.0 / (var.sqrt() + eps) if mutant == "eps_outside_sqrt" else torch.rsqrt(var + eps)
    if mutant == "affine_chunk_shifted" and NCH > 1:
        gv, bv = torch.roll(gv, 1, 0), torch.roll(bv, 1, 0)
    xh = (xv - mean[:, None, :, None]) * rstd[:, None, :, None]
    if mutant == "normalised_rounded_before_affine":
        xh = xh.to(dtype).float()
    y = _fma(xh, gv, bv).to(dtype)
    return y.view(rows, P)[:, :C].reshape(shape)


def merge_gather(x4d, mutant=None):
    """the kernel's index arithmetic (layernorm.hip:82-98): [B, H, W, Cs] -> [B, H2 W2, 4 Cs]"""
    assert mutant is None or mutant in MERGE_MUTANTS
    B, H, W, Cs = x4d.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    dev = x4d.device
    row = torch.arange(B * H2 * W2, device=dev)
    mb = row // (H2 * W2)
    rr = row - mb * H2 * W2
    Wd = W if mutant == "row_decode_uses_W_not_W2" else W2
    my = rr // Wd
    mx = rr - my * Wd
    k = torch.arange(4, device=dev)
    ky, kx = (k & 1, k >> 1) if mutant == "swap_ky_kx" else (k >> 1, k & 1)
    sy, sx = 2 * my[:, None] + ky[None], 2 * mx[:, None] + kx[None]
    if mutant == "pad_clamps_instead_of_zero":
        sy, sx = sy.clamp(max=H - 1), sx.clamp(max=W - 1)
    valid = (sy < H) & (sx < W)
    idx = torch.where(valid, (mb[:, None] * H + sy) * W + sx, torch.zeros_like(sy))
    got = x4d.reshape(B * H * W, Cs)[idx]                                                               # [rows, 4, Cs]
    got = torch.where(valid[..., None], got, torch.zeros_like(got))
    return got.reshape(B, H2 * W2, 4 * Cs)


def emulate_patch_merge_layernorm(x4d, gamma, beta, eps, mutant=None):
    if mutant in MERGE_MUTANTS:
        return emulate_layernorm(merge_gather(x4d, mutant), gamma, beta, eps)
    return emulate_layernorm(merge_gather(x4d), gamma, beta, eps, mutant)


def emulate_groupnorm_tokens(x, gamma, beta, groups, eps, mutant=None, pivot="first_mean", dest=None, row_start=0):
    """x [B, HW, C] 16-bit -> y [B, HW, C]; with dest [B, S, C]: a copy of dest with y written to rows row_start .. of each image.
    pivot: the K of the second sums ("first_mean": the float mean of the first reduction; None: the groups are never flagged)"""
    assert mutant is None or mutant in GN_MUTANTS
    dtype, f, dev = x.dtype, torch.float32, x.device
    B, HW, C = x.shape
    rows_par = GN_THREADS // groups
    R = -(-SLAB // rows_par)
    nslab = -(-HW // SLAB)
    # [B, nslab, R, rows_par, groups, 8]: row r0 + rpar + k rows_par of a slab is [k, rpar]
    xp = torch.zeros(B, nslab, R * rows_par, groups, 8, dtype=f, device=dev)
    local = torch.arange(R * rows_par, device=dev)
    glob = torch.arange(nslab, device=dev)[:, None] * SLAB + local[None]                                # [nslab, R rows_par]
    real = (local[None] < SLAB) & (glob < HW)
    xv = x.float().view(B, HW, groups, 8)
    xp[:, real] = xv[:, glob[real]]
    xp = xp.view(B, nslab, R, rows_par, groups, 8)
    real = real.view(1, nslab, R, rows_par, 1)
    zero = torch.zeros(B, nslab, rows_par, groups, dtype=f, device=dev)
    count = float(nslab * SLAB * 8 if mutant == "count_uses_full_slabs" else HW * 8)

    def reduce(K):
        """fp32 partials of x - K (K [B, groups] fp32) in the kernel's order, then fp64: (s / n, q / n)"""
        s, q = zero, zero
        for k in range(R):                                                                              # the lane's chain
            for e in range(8):
                v = xp[:, :, k, :, :, e] - K.view(B, 1, 1, groups)
                s = torch.where(real[:, :, k], s + v, s)
                q = torch.where(real[:, :, k], _fma(v, v, q), q)
        ts, tq = zero[:, :, 0], zero[:, :, 0]
        for p in range(rows_par):                                                                       # the LDS adds
            ts, tq = ts + s[:, :, p], tq + q[:, :, p]
        ts, tq = ts.double(), tq.double()                                                               # [B, nslab, groups]
        if mutant == "last_slab_dropped":
            ts, tq = ts[:, :-1], tq[:, :-1]
        return ts.sum(1) / count, tq.sum(1) / count

    eps = eps_f32(eps)
    mean, e2 = reduce(torch.zeros(B, groups, dtype=f, device=dev))
    var = (e2 - mean * mean).clamp_min(0.0)
    if mutant != "fp32_sums_no_pivot" and pivot is not None:
        n = gn_depth(groups)
        lost = E32 * ((n + 2) * e2 + 2 * (n + 1) * mean.abs() * e2.sqrt())
        flagged = lost > GN_RESUM[dtype] * (var + eps)
        if flagged.any():
            K = mean.float()
            m, e2k = reduce(K)
            mean = torch.where(flagged, K.double() + m, mean)
            var = torch.where(flagged, (e2k - m * m).clamp_min(0.0), var)
    if mutant == "group_spans_16_channels" and groups > 1:                                              # float64: no kernel to mirror
        pair = x.double().view(B, HW, groups // 2, 16)
        mean = pair.mean((1, 3)).repeat_interleave(2, 1)
        var = pair.var((1, 3), unbiased=False).repeat_interleave(2, 1)
    rstd = 1.0 / (var.sqrt() + eps) if mutant == "eps_outside_sqrt" else (var + eps) ** -0.5
    mean, rstd = mean.float(), rstd.float()
    if mutant == "stats_of_previous_image":
        mean, rstd = torch.roll(mean, 1, 0), torch.roll(rstd, 1, 0)
    xh = (xv - mean.view(B, 1, groups, 1)) * rstd.view(B, 1, groups, 1)
    y = _fma(xh, gamma.float().view(groups, 8), beta.float().view(groups, 8)).to(dtype).view(B, HW, C)
    if dest is None:
        return y
    out = dest.clone()
    flat = out.view(-1)
    stride = HW * C if mutant == "dest_ignores_batch_stride" else dest.shape[1] * C
    for b in range(B):
        flat[row_start * C + b * stride:row_start * C + b * stride + HW * C] = y[b].reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _affine(C, dtype, g, device, spread=0.2):
    gamma = (1 + spread * torch.randn(C, generator=g)).to(dtype)
    beta = (0.3 * torch.randn(C, generator=g)).to(dtype)
    return gamma.to(device), beta.to(device)


# C just past every dispatch edge of `launch` (nch = 1, 33, 65, 129, 193, 257, 385, 512), then the model's
LN_EDGE_C = [8, 264, 520, 1032, 1544, 2056, 3080, 4096]
LN_MODEL_C = [192, 256, 384, 768, 1536, 3072]
LN_ROWS = [1, 7, 33]
# one grid-stride case per lane-group width: 4096 workgroups x (256 / G) rows is the whole grid
LN_GRID_STRIDE = [(32768 + 9, 8), (16384 + 5, 264)]
# (rows, C) of the random cases tests/test_layernorm_gpu.py held to `ln_legacy_tol` before this module existed
LN_LEGACY = [(1, 8), (7, 192), (1000, 256), (513, 384), (300, 768), (77, 1536), (33, 3072), (5, 4096), (153600, 192), (2, 1000)]
# (mean, sigma, dtype): rows with |mean| >> sigma
LN_OFFSET = [(100.0, 0.05, torch.float16), (100.0, 0.05, torch.bfloat16), (1000.0, 1.0, torch.float16),
             (-300.0, 0.5, torch.bfloat16)]


def ln_legacy_tol(ref, dtype):
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    return ulp * ref.abs() + 1e-5 + ulp * 1e-2


def ln_random(rows, C, dtype, device="cpu"):
    g = _gen(rows + C)
    x = (torch.randn(rows, C, generator=g) * 3 + 1.5).to(dtype)
    return (x.to(device),) + _affine(C, dtype, g, device)


def ln_offset(mean, sigma, dtype, device="cpu", rows=64, C=256):
    g = _gen(int(abs(mean)))
    x = (mean + sigma * torch.randn(rows, C, generator=g)).to(dtype)
    return x.to(device), torch.ones(C, dtype=dtype, device=device), torch.zeros(C, dtype=dtype, device=device)


LN_CONSTANTS = [1.5, -3.25, 96.0, 0.0078125, -0.5, 7.0]         # <= 8 significant bits: exact in both types


def ln_constant(C, dtype, device="cpu"):
    """every row a constant: x - mean = 0 wherever the row sum and its product with 1/C are exact (C a power of two), so
    y == beta bit for bit; elsewhere the rounded 1/C shows, inside the bound"""
    g = _gen(C)
    x = torch.tensor(LN_CONSTANTS).view(-1, 1).expand(-1, C).contiguous().to(dtype)
    return (x.to(device),) + _affine(C, dtype, g, device)


LN_TWO_VALUED = [(0.0625, 2.0 ** -8), (3.0, 0.5), (-1.0, 2.0 ** -7), (0.0, 2.0 ** -8)]     # (m, d): m +- d exact in both types


def ln_two_valued(C, dtype, device="cpu"):
    """row i is m_i + d_i (-1)^j with gamma a signed power of two and beta = 0: mean m, variance d^2, and
    y = gamma (-1)^j d / sqrt(d^2 + eps) -- the only cases where eps (1e-5 against d^2 = 1.5e-5) decides the result"""
    g = _gen(C + 1)
    sign = 1.0 - 2.0 * (torch.arange(C) % 2)
    x = torch.stack([m + d * sign for m, d in LN_TWO_VALUED]).to(dtype)
    gamma = (2.0 ** torch.randint(-2, 3, (C,), generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, (C,), generator=g))
    return x.to(device), gamma.to(dtype).to(device), torch.zeros(C, dtype=dtype, device=device)


def ln_two_valued_expected(C, gamma, eps):
    sign = (1.0 - 2.0 * (torch.arange(C, device=gamma.device) % 2)).double()
    rows = [sign * d / math.sqrt(d * d + eps_f32(eps)) for _, d in LN_TWO_VALUED]
    return torch.stack(rows) * gamma.double()


LN_LAST_CHUNK_C = [264, 1032, 4096]


def ln_last_chunk(C, dtype, device="cpu"):
    """zero rows but for the last 16-byte chunk"""
    g = _gen(C + 2)
    x = torch.zeros(3, C)
    x[:, -8:] = torch.randint(1, 9, (3, 8), generator=g).float()
    return (x.to(dtype).to(device),) + _affine(C, dtype, g, device)


def ln_last_chunk_expected(x, gamma, beta, eps):
    """closed form: with v the last eight values, mean = sum v / C, var = sum v^2 / C - mean^2; every zero gives
    -mean rstd gamma + beta"""
    C = x.shape[-1]
    v = x[:, -8:].double()
    mean = v.sum(-1, keepdim=True) / C
    rstd = ((v * v).sum(-1, keepdim=True) / C - mean * mean + eps_f32(eps)) ** -0.5
    xhat = torch.cat([(-mean * rstd).expand(-1, C - 8), (v - mean) * rstd], -1)
    return xhat * gamma.double() + beta.double()


MERGE_SHAPES = [(1, 1, 1, 8), (2, 7, 9, 192), (1, 8, 12, 96), (1, 5, 6, 64), (2, 3, 2, 1024)]
MERGE_LEGACY_BF16 = (2, 14, 10, 96)             # held to rtol 1e-2, atol 2e-2 before


def merge_input(B, H, W, Cs, dtype, device="cpu"):
    """a token map whose every source pixel has its own mean and spread: a mis-routed gather changes a row's statistics"""
    g = _gen(1000 * H + 10 * W + Cs)
    mean = 2.0 * torch.randn(B, H, W, 1, generator=g)
    spread = 0.5 + 1.5 * torch.rand(B, H, W, 1, generator=g)
    x = (mean + spread * torch.randn(B, H, W, Cs, generator=g)).to(dtype)
    gamma = (1 + 0.1 * torch.randn(4 * Cs, generator=g)).to(dtype)
    beta = (0.1 * torch.randn(4 * Cs, generator=g)).to(dtype)
    return x.to(device), gamma.to(device), beta.to(device)


GN_GROUPS = [1, 2, 32, 64, 256]                 # C = 8 .. 2048, rows_par = 256 .. 1
GN_HW = [1, 127, 128, 129, 300]
GN_B = 3
# (mean, sigma) per type.  bf16 steps are 0.5 at 100 and 4 at 1000: the twin of 100 +- 0.05 takes sigma = 0.1, which leaves
# {99.5, 100, 100.5} (tests/test_norm_bounds_cpu.py checks that three values survive in every group)
GN_OFFSET = {torch.float16: [(0.7, 2.0), (8.0, 1.0), (32.0, 1.0), (100.0, 1.0), (100.0, 0.25), (1000.0, 1.0), (100.0, 0.05)],
             torch.bfloat16: [(0.7, 2.0), (8.0, 1.0), (32.0, 1.0), (100.0, 1.0), (100.0, 0.25), (1000.0, 1.0), (100.0, 0.1)]}
GN_OFFSET_MUST_CATCH = {torch.float16: [(100.0, 0.25), (100.0, 0.05)], torch.bfloat16: [(100.0, 0.25), (100.0, 0.1)]}
# (B, H W) of the C = 256 cases tests/test_groupnorm_gpu.py held to 2^-10 |ref| + 2e-3 (fp16) before; bf16: rtol 1e-2, atol 2e-2
GN_LEGACY_F16 = [(1, 1), (2, 63), (1, 9600), (3, 561), (1, 153600)]
GN_LEGACY_BF16 = (2, 777)


def gn_random(groups, HW, dtype, device="cpu", B=GN_B):
    """a different mean and spread per image and per group"""
    g, C = _gen(1000 * groups + HW), groups * 8
    mean = 2.0 * torch.randn(B, 1, groups, 1, generator=g)
    spread = 0.5 + 1.5 * torch.rand(B, 1, groups, 1, generator=g)
    x = (mean + spread * torch.randn(B, HW, groups, 8, generator=g)).view(B, HW, C).to(dtype)
    return (x.to(device),) + _affine(C, dtype, g, device)


def gn_legacy(B, HW, dtype, device="cpu"):
    g, C = _gen(HW), 256
    x = (torch.randn(B, HW, C, generator=g) * 2 + 0.7).to(dtype)
    return (x.to(device),) + _affine(C, dtype, g, device)


def gn_offset(mean, sigma, dtype, device="cpu", B=GN_B, HW=300, groups=32):
    g, C = _gen(int(mean * 100 + sigma * 1000)), groups * 8
    x = (mean + sigma * torch.randn(B, HW, C, generator=g)).to(dtype)
    return (x.to(device),) + _affine(C, dtype, g, device)


def gn_outlier(dtype, device="cpu", B=GN_B, HW=300, groups=32):
    """token 0 of every image sits 50 sigma from its group's mean: the worst input for a pivot taken from token 0 (the kernel's
    pivot is the first mean, which an outlier cannot own)"""
    g, C = _gen(50), groups * 8
    mean = 2.0 * torch.randn(B, 1, groups, 1, generator=g)
    spread = 0.5 + 1.5 * torch.rand(B, 1, groups, 1, generator=g)
    x = mean + spread * torch.randn(B, HW, groups, 8, generator=g)
    x[:, 0] = (mean + 50 * spread)[:, 0]
    return (x.view(B, HW, C).to(dtype).to(device),) + _affine(C, dtype, g, device)


def gn_constant(dtype, device="cpu", B=GN_B, HW=129, groups=32):
    """every (image, group) a constant of <= 8 significant bits: the first sums are exact, var + eps = eps flags the group, K is
    the constant, every second sum is 0, y == beta bit for bit"""
    g, C = _gen(3), groups * 8
    c = (torch.arange(B).view(B, 1, 1, 1) + 1) * (torch.arange(groups).view(1, 1, groups, 1) - 16) / 4.0
    x = c.expand(B, HW, groups, 8).reshape(B, HW, C).to(dtype)
    return (x.to(device),) + _affine(C, dtype, g, device)


def _gn_two_valued_md(B, groups):
    m = ((torch.arange(groups) % 5) - 2).view(1, 1, groups, 1) * 0.25
    d = (2.0 ** (torch.arange(B) - 8.0)).view(B, 1, 1, 1)
    return m, d


def gn_two_valued(dtype, device="cpu", B=GN_B, HW=129, groups=32):
    """group g of image b holds m_g + d_b (-1)^channel: mean m, variance d^2 (2^-16 .. 2^-12 against eps = 1e-5),
    xhat = +-d / sqrt(d^2 + eps)"""
    g, C = _gen(4), groups * 8
    m, d = _gn_two_valued_md(B, groups)
    sign = (1.0 - 2.0 * (torch.arange(8) % 2)).view(1, 1, 1, 8)
    x = (m + d * sign).expand(B, HW, groups, 8).reshape(B, HW, C).to(dtype)
    return (x.to(device),) + _affine(C, dtype, g, device)


def gn_two_valued_expected(gamma, beta, eps, B=GN_B, HW=129, groups=32):
    _, d = _gn_two_valued_md(B, groups)
    d = d.double().to(gamma.device)
    sign = (1.0 - 2.0 * (torch.arange(8, device=gamma.device) % 2)).double().view(1, 1, 1, 8)
    xhat = (sign * d / torch.sqrt(d * d + eps_f32(eps))).expand(B, HW, groups, 8)
    return xhat * gamma.double().view(groups, 8) + beta.double().view(groups, 8)
