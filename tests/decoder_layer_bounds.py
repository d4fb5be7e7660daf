"""float64 reference, derived interval bound, CPU emulation with mutants, weight packing and test inputs for
codetr_decoder_layer_{f16,bf16} (csrc/decoder_layer.hip).  Pure torch: the same code runs on the CPU and on the device;
tests/test_decoder_layer_bounds_cpu.py proves the cases and the mutant table, tests/test_decoder_layer_bounds_gpu.py runs the
kernel.

What the kernel computes.  E rounds to the storage type (fp16 / bf16) and stands exactly where the kernel rounds; line numbers
are those of decoder_layer.hip.  A workgroup owns 16 rows, a row's image is row / Nq, rows past `rows` are clamped for loads and
masked for stores.

TAIL (skipped in the first launch of a decoder):

    t1 = E(E(Wo attn + bo) + x)                      :430
    x1 = E(LN1(t1));  q2 = E(x1 + qpos)              :441-442
    pj = E(Wol q2 + bol)                             :465   columns: offsets [m][l][p][xy], then logits [m][l*P + p]
    s  = E(MSDA)                                     :472-581, fp32 throughout:
           softmax over the L*P logits of a (row, head) with the fast exp
           sig = 1 / (1 + expf(-ref))
           (rx, ry, rw, rh) = sig * vr32[b, l, (0, 1, 0, 1)]
           loc = off * (wh * 0.5 / P) + xy
           im = fma(loc, size, -0.5)
           gate: -1 < im < size
           corners masked by h0 >= 0, w0 >= 0, h0 + 1 <= H - 1, w0 + 1 <= W - 1
           fp32 fma of weight * value over L*P * 4 corners
    t2 = E(E(Wout s + bout) + x1);  x2 = E(LN2(t2))  :597, :605
    h  = E(relu(W1 x2 + b1))   per 256-wide chunk    :626
           workgroup g walks chunk (c + ((g >> 3) & 7)) & 7 at step c   :191, :393, :623
    y32 = W2 h + b2 + x2        kept in fp32, NOT rounded   :641
    x3 = E(LN3(y32))                                 :650
    out = E(LNf(x3))            only when no HEAD follows   :660
    r1 = E(relu(Wr1 x3 + br1)), r2 = E(relu(Wr2 r1 + br2))
    ref' = E(E(Wr3 r2 + br3) + ref)                  :702

HEAD (for a HEAD-only launch, x3 = x and ref' = ref):

    v0[c]  = sigmoid(ref'[c]) * vr32[b, level 0, c & 1]
    sine   = E(sin | cos), blocks ordered (y, x, w, h)        :716-737
    p1     = E(relu(Wp1 sine + bp1))
    qpos'  = E(Wp2 p1 + bp2)
    q_in   = E(x3 + qpos')                                    :754, :768-769
    qk     = E(Wqk q_in + bqk)
    v      = E(Wv x3 + bv)

`exact(inp)` walks this in float64 on the 16-bit inputs.  `bound(ex)` carries tests/ffn_bounds.py's interval radius (its `_prod`,
`_add`, `_relu`, `_rnd`, `_norm` and norm_bounds.bound_layernorm) through the TAIL up to x_out.  It is meant for the probe cases
below, where at most the LayerNorms and one product are inexact, and stays within a few steps of the storage type there; the
gather contributes a radius only where its inputs (pj) are exact -- then 2^-24 (4 L P + 64) sum |weight| |value|, every fp32
operation between a logit and the sum -- and the bound is inf behind a gather whose inputs carry a radius.  For the full random
layer it promises nothing and is not used there (ffn_bounds.py says the same of its oproj form).

`emulate(inp, mutant=None)` repeats the kernel's rounding points in fp32 torch (any summation order); `mutant` is one of
DEC_MUTANTS, the errors the cases exist to catch.  `pack(inp)` builds the four weight blobs through
DinoTransformerDecoder._fused_weights on a module whose parameters were set from `inp`, so the product's own packing
(pack_fragment_major, the vector order) is under test too; `unpack` inverts the layout include/codetr_hip.h documents.

Cases (`CASE_NAMES`, `build`, `hold`): 111 rows (B = 3, Nq = 37: tiles span two images, the last tile is partial) on a five-level
pyramid with an H == 1 and a W == 1 level, cut to L levels.

    gather_exact_L*P*   x1 = 0, one-hot qpos: row r reads its own table of dyadic offsets and 0 / -30000 logits from column r of
                        Wol; integer value map; signed-permutation Wout; x_out = E(LN(E(LN(exact)))) within `bound`
    oproj_exact         integers either side of the largest one the type counts to; three chained LayerNorms within `bound`
    ffn_exact           921 rows (all eight chunk rotations), x2 = beta2: every row of x_out equals row 0, row 0 within `bound`
    ffn_rounding        y32 = 4096 + small integers through hidden values that E moves: the hidden rounding, the fp32 rows in
                        front of LN3 and the two-pass variance, within `bound` (products of integers below 2^24 are exact in
                        fp32 in any order: `_prod` drops the accumulation radius there)
    box_exact_*         x3 = beta3: ref_out, v_out (TAIL + HEAD) and the output norm (TAIL alone) bit for bit
    sine_exact          HEAD alone, Wp1 = +-selection, Wp2 = 1: qpos_out holds relu(+-E(sine)); against float64 at u + 1e-3
    random_L*P*_*       trained-like scales: helpers_model.assert_rows_close at 3e-3 (x 8 for bf16) against float64 per output,
                        and err(kernel) <= 1.5 err(emulation) + 1e-3 (x 8) in relative L2

An `inp` is a dict of plain tensors: the activations x, attn, qpos [rows, 256], ref [rows, 4], vr32 [B, L, 2] fp32, the value map
[B, S, 8, 32], the weights under the names of `weight_shapes`, and dtype, L, P, shapes, B, Nq, tail, head, eps, temperature.
Inputs come from a CPU generator (the same values on every machine).
"""
import collections
import math

import torch

import ffn_bounds as fb
import norm_bounds as nb

E32 = nb.E32
C, M, D, F = 256, 8, 32, 2048
ROWS_PER_WG = 16
MAX_L, MAX_LP = 8, 20
# an H == 1 and a W == 1 level; level 0 has power-of-two sides so that a dyadic offset reaches im = -1, size - 1 and size on
# both axes at every L (on a side of 3, im = -1 is loc = -1/6)
PYRAMID = [(4, 8), (3, 4), (2, 2), (1, 3), (2, 1)]
LP_PROBES = ((5, 4), (4, 4), (3, 4), (5, 2), (1, 2), (2, 8))  # gather_exact and random
LP_RANDOM = LP_PROBES + ((4, 5),)                             # 0.5 / 5 is not dyadic: the random case only
INT_LIMIT = fb.INT_LIMIT
U = nb.U

DEC_MUTANTS = (
    # gather
    "corner_index_transposed", "level_start_ignored", "row_image_is_tile_image", "gate_inclusive", "border_corner_kept",
    "offset_xy_swapped", "offset_scale_without_half", "wh_taken_from_xy", "valid_ratio_of_level0_everywhere",
    "softmax_per_level", "logit_columns_point_major", "points_beyond_ten_dropped", "head_stride_wrong",
    # products / norms
    "oproj_not_rounded_before_residual", "q2_without_qpos", "b1_chunk_not_rotated", "w2_chunk_not_rotated",
    "last_chunk_dropped", "hidden_kept_fp32", "pre_ln3_rounded", "ffn_residual_is_x1", "one_pass_variance",
    "final_norm_skipped",
    # boxes / head
    "ref_added_before_rounding", "sine_xy_order", "sine_uses_own_level_ratio", "sine_of_unrefined_ref",
    "temperature_natural_log", "k_without_qpos", "v_with_qpos")

Exact = collections.namedtuple("Exact", "x_out ref_out qpos_out qk_out v_out stages inp")
Outputs = collections.namedtuple("Outputs", "x_out ref_out qpos_out qk_out v_out")
OUTPUT_WIDTH = dict(x_out=C, ref_out=4, qpos_out=C, qk_out=2 * C, v_out=C)


def supported(L, P):
    """what dims_ok states of (num_levels, num_points): the (offsets | logits) projection has 24 L P columns in tiles of 16, at
    most 512 of them"""
    return 1 <= L <= MAX_L and P >= 1 and (L * P) % 2 == 0 and L * P <= MAX_LP


def weight_shapes(L, P):
    LP = L * P
    return dict(wo=(C, C), bo=(C,), g1=(C,), e1=(C,), woff=(M * LP * 2, C), boff=(M * LP * 2,), wlog=(M * LP, C), blog=(M * LP,),
                wout=(C, C), bout=(C,), g2=(C,), e2=(C,), w1=(F, C), b1=(F,), w2=(C, F), b2=(C,), g3=(C,), e3=(C,),
                wr1=(C, C), br1=(C,), wr2=(C, C), br2=(C,), wr3=(4, C), br3=(4,),
                wp1=(C, 2 * C), bp1=(C,), wp2=(C, C), bp2=(C,), wqk=(2 * C, C), bqk=(2 * C,), wv=(C, C), bv=(C,),
                gf=(C,), ef=(C,))


def level_starts(shapes):
    out, o = [], 0
    for h, w in shapes:
        out.append(o)
        o += h * w
    return out, o


def rotation(rows, device="cpu"):
    """[rows]: the chunk rotation (g >> 3) & 7 of the workgroup g = row / 16 that owns the row"""
    return ((torch.arange(rows, device=device) // ROWS_PER_WG) >> 3) & 7


# ------------------------------------------------------------------------------------------------------- the gather and the sine
def _levels(inp, device):
    shapes = inp["shapes"]
    starts, S = level_starts(shapes)
    lvl = torch.arange(inp["L"] * inp["P"], device=device) // inp["P"]
    Hs = torch.tensor([h for h, _ in shapes], device=device)[lvl]
    Ws = torch.tensor([w for _, w in shapes], device=device)[lvl]
    st = torch.tensor(starts, device=device)[lvl]
    return lvl, Hs, Ws, st, S


def gather(inp, pj, ref, f, mutant=None, magnitude=False, geometry=None):
    """s [rows, 256] in arithmetic of type f (float64: the reference; float32: the emulation) from the rounded projection pj
    [rows, 24 L P] and the unactivated boxes ref [rows, 4]: the kernel's formulation, corner masks and clamped indices included
    (under the exclusive gate they are the zero padding of bilinear sampling).  magnitude: sum |weight| |value| instead.
    geometry: a dict that receives h_im, w_im [rows, 8, L P] and the attention weights"""
    L, P, Nq = inp["L"], inp["P"], inp["Nq"]
    LP, R, dev = L * P, pj.shape[0], pj.device
    lvl, Hi, Wi, st, S = _levels(inp, dev)
    rows = torch.arange(R, device=dev)
    b = (rows // ROWS_PER_WG * ROWS_PER_WG) // Nq if mutant == "row_image_is_tile_image" else rows // Nq
    off = pj[:, :M * LP * 2].to(f).view(R, M, LP, 2)
    lg = pj[:, M * LP * 2:M * LP * 3].to(f).view(R, M, LP)
    if mutant == "logit_columns_point_major":
        lg = lg.view(R, M, P, L).transpose(2, 3).reshape(R, M, LP)
    if mutant == "softmax_per_level":
        aw = torch.softmax(lg.view(R, M, L, P), -1).view(R, M, LP)
    else:
        aw = torch.softmax(lg, -1)
    if mutant == "points_beyond_ten_dropped":
        aw = torch.cat([aw[..., :10], torch.zeros_like(aw[..., 10:])], -1)
    px, py = (off[..., 1], off[..., 0]) if mutant == "offset_xy_swapped" else (off[..., 0], off[..., 1])
    sig = 1.0 / (1.0 + torch.exp(-ref.to(f)))                                                   # [R, 4]
    vr = inp["vr32"].to(f)[b]                                                                  # [R, L, 2]
    if mutant == "valid_ratio_of_level0_everywhere":
        vr = vr[:, :1].expand(-1, L, -1)
    vrx, vry = vr[:, lvl, 0], vr[:, lvl, 1]                                                     # [R, LP]
    rx, ry, rw, rh = sig[:, 0:1] * vrx, sig[:, 1:2] * vry, sig[:, 2:3] * vrx, sig[:, 3:4] * vry
    if mutant == "wh_taken_from_xy":
        rw, rh = rx, ry
    k = torch.tensor((1.0 if mutant == "offset_scale_without_half" else 0.5), dtype=f, device=dev) / torch.tensor(float(P), dtype=f, device=dev)
    x = px * (rw * k)[:, None] + rx[:, None]
    y = py * (rh * k)[:, None] + ry[:, None]
    Hf, Wf = Hi.to(f), Wi.to(f)
    h_im, w_im = y * Hf - 0.5, x * Wf - 0.5
    if mutant == "gate_inclusive":
        gate = (h_im >= -1) & (w_im >= -1) & (h_im <= Hf) & (w_im <= Wf)
    else:
        gate = (h_im > -1) & (w_im > -1) & (h_im < Hf) & (w_im < Wf)
    if geometry is not None:
        geometry.update(h_im=h_im, w_im=w_im, aw=aw, gate=gate)
    big = 1 << 20                                                                              # far outside: keep floor() inside int64
    hf, wf = torch.floor(h_im.clamp(-big, big)), torch.floor(w_im.clamp(-big, big))
    lh, lw = h_im.clamp(-big, big) - hf, w_im.clamp(-big, big) - wf
    h0, w0 = hf.long(), wf.long()
    top = 0 if mutant == "border_corner_kept" else 1
    oks = {(0, 0): (h0 >= 0) & (w0 >= 0), (0, 1): (h0 >= 0) & (w0 + 1 <= Wi - top),
           (1, 0): (h0 + 1 <= Hi - top) & (w0 >= 0), (1, 1): (h0 + 1 <= Hi - top) & (w0 + 1 <= Wi - top)}
    value = inp["value"].to(f)
    if magnitude:
        value, aw = value.abs(), aw.abs()
    vflat = value.reshape(value.shape[0], S, M * D)
    ch = torch.arange(D, device=dev)[None] + (D // 2 if mutant == "head_stride_wrong" else D) * torch.arange(M, device=dev)[:, None]
    ch = ch % (M * D)                                                                          # [M, D]
    out = torch.zeros(R, M, D, dtype=f, device=dev)
    g_aw = torch.where(gate, aw, torch.zeros_like(aw))
    for (dy, dx), ok in oks.items():
        wy, wx = (lh if dy else 1.0 - lh), (lw if dx else 1.0 - lw)
        hc, wc = (h0 + dy).clamp(min=0).minimum(Hi - 1), (w0 + dx).clamp(min=0).minimum(Wi - 1)
        flat = wc * Hi + hc if mutant == "corner_index_transposed" else hc * Wi + wc
        if mutant != "level_start_ignored":
            flat = flat + st
        wgt = torch.where(ok, wy * wx * g_aw, torch.zeros_like(g_aw))                           # [R, M, LP]
        samp = vflat[b[:, None, None, None], flat[..., None], ch[None, :, None, :]]             # [R, M, LP, D]
        out = out + (wgt[..., None] * samp).sum(2)
    return out.reshape(R, M * D)


def sine(inp, ref, f, mutant=None):
    """[rows, 512] sin | cos of the level-0 reference box, unrounded, in arithmetic of type f"""
    R, dev, L = ref.shape[0], ref.device, inp["L"]
    b = torch.arange(R, device=dev) // inp["Nq"]
    lev = min(1, L - 1) if mutant == "sine_uses_own_level_ratio" else 0
    vr0 = inp["vr32"].to(f)[b, lev]                                                            # [R, 2]
    v0 = (1.0 / (1.0 + torch.exp(-ref.to(f)))) * vr0[:, [0, 1, 0, 1]]
    fr = torch.arange(C // 4, dtype=f, device=dev)                                             # 64 (sin, cos) pairs per coordinate
    T = math.log(inp["temperature"]) if mutant == "temperature_natural_log" else math.log2(inp["temperature"])
    inv = torch.exp2(-T * (2.0 * fr / (C // 2)))
    ang = (v0 * (2.0 * math.pi))[:, :, None] * inv                                             # [R, 4, 64]
    emb = torch.stack((ang.sin(), ang.cos()), -1).flatten(-2)                                  # [R, 4, 128]
    order = [0, 1, 2, 3] if mutant == "sine_xy_order" else [1, 0, 2, 3]
    return emb[:, order].reshape(R, 2 * C)


# ------------------------------------------------------------------------------------------------------- float64 and intervals
def _norm_wide(v, r, ln, dt, track):
    """ffn_bounds._norm for an input that is NOT a value of the storage type (the fp32 rows in front of LN3)"""
    g, b, eps = ln
    xd, gd, bd, eps = v, g.double(), b.double(), nb.eps_f32(eps)
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xhat = (xd - mu) * rstd
    ex = nb.Exact(xhat * gd + bd, mu, var, rstd, xhat, xd, gd, bd, eps, dt)
    if not track:
        return ex.out, None
    n_s = v.shape[-1] // 4 + 2
    fp32 = nb.bound_layernorm(ex, n_s).fp32
    d = r + r.mean(-1, keepdim=True)
    dv = 2 * ((ex.x - ex.mu).abs() * d).mean(-1, keepdim=True) + (d * d).mean(-1, keepdim=True)
    rel = nb._rsqrt_rel(dv / (ex.var + ex.eps))
    lost = torch.isinf(rel)
    rel = rel.masked_fill(lost, 0.0)
    sens = ex.gamma.abs() * (d * ex.rstd * (1 + rel) + ex.xhat.abs() * rel)
    return ex.out, (fp32 * (1 + rel) + sens * (1 + E32 * (n_s + 7))).masked_fill(lost.expand_as(sens), math.inf)


def _prod(a, ra, w, bias, track):
    """ffn_bounds._prod; where the row, the matrix and the bias are integers, the row carries no radius and sum |w| |a| + |bias|
    stays below 2^24, every partial sum in any order is an integer that fp32 holds: the accumulation adds nothing"""
    pre, r = fb._prod(a, ra, w, bias, track)
    if not track:
        return pre, r
    whole = bool((w == w.round()).all()) and bool((bias == bias.round()).all())
    rows_ok = (a == a.round()).all(-1, keepdim=True) & (a.abs() @ w.abs().t() + bias.abs() < 2.0 ** 24)
    if torch.is_tensor(ra):
        rows_ok = rows_ok & (ra == 0).all(-1, keepdim=True)
    return pre, torch.where(rows_ok & whole, torch.zeros_like(r), r)


def _walk(inp, track):
    dt, eps = inp["dtype"], inp["eps"]
    Dd = lambda k: inp[k].double()   # noqa: E731
    zero = 0.0 if track else None
    st, r_out = {}, None
    if inp["tail"]:
        v, r = fb._rnd(*_prod(Dd("attn"), zero, Dd("wo"), Dd("bo"), track), dt)
        t1, r = fb._rnd(*fb._add(v, r, Dd("x"), zero, track), dt)
        x1, r1 = fb._rnd(*fb._norm(t1, r, (inp["g1"], inp["e1"], eps), dt, track), dt)
        q2, rq = fb._rnd(*fb._add(x1, r1, Dd("qpos"), zero, track), dt)
        wol, bol = torch.cat((Dd("woff"), Dd("wlog")), 0), torch.cat((Dd("boff"), Dd("blog")), 0)
        pj, rp = fb._rnd(*_prod(q2, rq, wol, bol, track), dt)
        geo = {}
        s64 = gather(inp, pj, inp["ref"], torch.float64, geometry=geo)
        rs = None
        if track:
            if float(rp.max()) == 0.0:
                rs = E32 * (4 * inp["L"] * inp["P"] + 64) * gather(inp, pj, inp["ref"], torch.float64, magnitude=True)
            else:
                rs = torch.full_like(s64, math.inf)
        s, rs = fb._rnd(s64, rs, dt)
        v, r = fb._rnd(*_prod(s, rs, Dd("wout"), Dd("bout"), track), dt)
        t2, r = fb._rnd(*fb._add(v, r, x1, r1, track), dt)
        x2, r2 = fb._rnd(*fb._norm(t2, r, (inp["g2"], inp["e2"], eps), dt, track), dt)
        h, rh = fb._relu(*fb._rnd(*_prod(x2, r2, Dd("w1"), Dd("b1"), track), dt))
        y, ry = _prod(h, rh, Dd("w2"), Dd("b2"), track)
        y32, ry = fb._add(y, ry, x2, r2, track)
        x3, r3 = fb._rnd(*_norm_wide(y32, ry, (inp["g3"], inp["e3"], eps), dt, track), dt)
        if inp["head"]:
            x_out, r_out = x3, r3
        else:
            x_out, r_out = fb._rnd(*fb._norm(x3, r3, (inp["gf"], inp["ef"], eps), dt, track), dt)
        E = lambda t: fb._E(t, dt)   # noqa: E731
        lin = lambda a, w, bb: a @ Dd(w).t() + Dd(bb)   # noqa: E731
        rr1 = E(lin(x3, "wr1", "br1")).clamp_min(0.0)
        rr2 = E(lin(rr1, "wr2", "br2")).clamp_min(0.0)
        delta = E(lin(rr2, "wr3", "br3"))
        ref_out = E(delta + Dd("ref"))
        st.update(t1=t1, x1=x1, q2=q2, pj=pj, s64=s64, s=s, t2=t2, x2=x2, h=h, y32=y32, x3=x3, r1=rr1, r2=rr2, delta=delta,
                  h_im=geo["h_im"], w_im=geo["w_im"], aw=geo["aw"], gate=geo["gate"])
    else:
        x3, x_out, ref_out = Dd("x"), None, Dd("ref")
    qpos_out = qk_out = v_out = None
    if inp["head"]:
        E = lambda t: fb._E(t, dt)   # noqa: E731
        lin = lambda a, w, bb: a @ Dd(w).t() + Dd(bb)   # noqa: E731
        sine64 = sine(inp, ref_out, torch.float64)
        sn = E(sine64)
        p1 = E(lin(sn, "wp1", "bp1")).clamp_min(0.0)
        qpos_out = E(lin(p1, "wp2", "bp2"))
        q_in = E(x3 + qpos_out)
        qk_out = E(lin(q_in, "wqk", "bqk"))
        v_out = E(lin(x3, "wv", "bv"))
        st.update(sine64=sine64, sine=sn, p1=p1, q_in=q_in)
    if not inp["tail"]:
        ref_out = None
    return Exact(x_out, ref_out, qpos_out, qk_out, v_out, st, inp), r_out


def exact(inp):
    """-> Exact(x_out, ref_out, qpos_out, qk_out, v_out (None where the launch form does not write them), stages, inp)"""
    return _walk(inp, False)[0]


def bound(ex):
    """[rows, 256]: the derived elementwise bound on |kernel x_out - ex.x_out|"""
    assert ex.inp["tail"]
    r = _walk(ex.inp, True)[1]
    return r.nan_to_num(nan=math.inf, posinf=math.inf)


ratio = fb.ratio


# ------------------------------------------------------------------------------------------------------- emulation
def _ln32(x, g, b, eps, one_pass):
    return fb._ln32(x, (g, b, eps), one_pass)


def emulate(inp, mutant=None):
    """-> Outputs in the storage type (None where the launch form does not write them)"""
    assert mutant is None or mutant in DEC_MUTANTS
    dt, eps = inp["dtype"], inp["eps"]
    R = lambda t: t.to(dt).float()   # noqa: E731
    Ff = lambda k: inp[k].float()   # noqa: E731
    lin = lambda a, w, bb: a @ Ff(w).t() + Ff(bb)   # noqa: E731
    one = mutant == "one_pass_variance"
    x_out = ref_out = qpos_out = qk_out = v_out = None
    if inp["tail"]:
        x, rows = Ff("x"), inp["x"].shape[0]
        if mutant == "oproj_not_rounded_before_residual":
            t1 = R(lin(Ff("attn"), "wo", "bo") + x)
        else:
            t1 = R(R(lin(Ff("attn"), "wo", "bo")) + x)
        x1 = R(_ln32(t1, inp["g1"], inp["e1"], eps, one))
        q2 = x1 if mutant == "q2_without_qpos" else R(x1 + Ff("qpos"))
        pj = R(q2 @ torch.cat((Ff("woff"), Ff("wlog")), 0).t() + torch.cat((Ff("boff"), Ff("blog")), 0))
        s = R(gather(inp, pj, inp["ref"], torch.float32, mutant))
        t2 = R(R(lin(s, "wout", "bout")) + x1)
        x2 = R(_ln32(t2, inp["g2"], inp["e2"], eps, one))
        # the FFN in the workgroups' chunk order: step c of workgroup g is hidden chunk (c + rot) & 7
        rot = rotation(rows, x.device)
        w1, b1, w2 = Ff("w1"), Ff("b1"), Ff("w2")
        y = torch.zeros(rows, C, dtype=torch.float32, device=x.device)
        for rv in rot.unique().tolist():
            sel = rot == rv
            xs = x2[sel]
            acc = torch.zeros(xs.shape[0], C, dtype=torch.float32, device=x.device)
            for c in range(8 - (1 if mutant == "last_chunk_dropped" else 0)):
                chk = (c + rv) & 7
                cb = c if mutant == "b1_chunk_not_rotated" else chk
                c2 = c if mutant == "w2_chunk_not_rotated" else chk
                hh = (xs @ w1[chk * 256:(chk + 1) * 256].t() + b1[cb * 256:(cb + 1) * 256]).clamp_min(0.0)
                if mutant != "hidden_kept_fp32":
                    hh = R(hh)
                acc = acc + hh @ w2[:, c2 * 256:(c2 + 1) * 256].t()
            y[sel] = acc
        y32 = y + Ff("b2") + (x1 if mutant == "ffn_residual_is_x1" else x2)
        if mutant == "pre_ln3_rounded":
            y32 = R(y32)
        x3 = R(_ln32(y32, inp["g3"], inp["e3"], eps, one))
        if inp["head"] or mutant == "final_norm_skipped":
            x_out = x3
        else:
            x_out = R(_ln32(x3, inp["gf"], inp["ef"], eps, one))
        r1 = R(lin(x3, "wr1", "br1").clamp_min(0.0))
        r2 = R(lin(r1, "wr2", "br2").clamp_min(0.0))
        if mutant == "ref_added_before_rounding":
            ref_new = R(lin(r2, "wr3", "br3") + Ff("ref"))
        else:
            ref_new = R(R(lin(r2, "wr3", "br3")) + Ff("ref"))
        ref_out = ref_new
    else:
        x3, ref_new = Ff("x"), Ff("ref")
    if inp["head"]:
        ref_sine = Ff("ref") if mutant == "sine_of_unrefined_ref" else ref_new
        sn = R(sine(inp, ref_sine, torch.float32, mutant))
        p1 = R(lin(sn, "wp1", "bp1").clamp_min(0.0))
        qpos_out = R(lin(p1, "wp2", "bp2"))
        q_in = R(x3 + qpos_out)
        qk_out = R(lin(q_in, "wqk", "bqk"))
        if mutant == "k_without_qpos":
            qk_out = torch.cat((qk_out[:, :C], R(lin(x3, "wqk", "bqk"))[:, C:]), 1)
        v_out = R(lin(q_in if mutant == "v_with_qpos" else x3, "wv", "bv"))
    to = lambda t: None if t is None else t.to(dt)   # noqa: E731
    return Outputs(to(x_out), to(ref_out), to(qpos_out), to(qk_out), to(v_out))


# ------------------------------------------------------------------------------------------------------- packing
def build_module(inp, device="cpu"):
    """(DinoTransformerDecoder of one layer, reg branches) with the parameters of `inp`, in its type, on `device`"""
    from codetr.transformer import DinoTransformerDecoder, build_MLP

    cfg = dict(type="DetrTransformerDecoderLayer",
               attn_cfgs=[dict(type="MultiheadAttention", embed_dims=C, num_heads=M, dropout=0.0),
                          dict(type="MultiScaleDeformableAttention", embed_dims=C, num_levels=inp["L"], num_points=inp["P"],
                               dropout=0.0)],
               feedforward_channels=F, ffn_dropout=0.0,
               operation_order=("self_attn", "norm", "cross_attn", "norm", "ffn", "norm"))
    dec = DinoTransformerDecoder(return_intermediate=True, transformerlayers=cfg, num_layers=1)
    reg = torch.nn.ModuleList([build_MLP(C, C, 4, 3)])
    layer = dec.layers[0]
    sa, ca, ffn = layer.attentions[0], layer.attentions[1], layer.ffns[0]
    n1, n2, n3 = layer.norms
    rb, rp = reg[0], dec.ref_point_head
    pairs = [(sa.attn.out_proj.weight, "wo"), (sa.attn.out_proj.bias, "bo"), (n1.weight, "g1"), (n1.bias, "e1"),
             (ca.sampling_offsets.weight, "woff"), (ca.sampling_offsets.bias, "boff"), (ca.attention_weights.weight, "wlog"),
             (ca.attention_weights.bias, "blog"), (ca.output_proj.weight, "wout"), (ca.output_proj.bias, "bout"),
             (n2.weight, "g2"), (n2.bias, "e2"), (ffn.layers[0][0].weight, "w1"), (ffn.layers[0][0].bias, "b1"),
             (ffn.layers[1].weight, "w2"), (ffn.layers[1].bias, "b2"), (n3.weight, "g3"), (n3.bias, "e3"),
             (rb[0].weight, "wr1"), (rb[0].bias, "br1"), (rb[2].weight, "wr2"), (rb[2].bias, "br2"), (rb[4].weight, "wr3"),
             (rb[4].bias, "br3"), (rp[0].weight, "wp1"), (rp[0].bias, "bp1"), (rp[2].weight, "wp2"), (rp[2].bias, "bp2"),
             (dec.norm.weight, "gf"), (dec.norm.bias, "ef")]
    with torch.no_grad():
        for p, k in pairs:
            p.copy_(inp[k].float())
        sa.attn.in_proj_weight.copy_(torch.cat((inp["wqk"], inp["wv"]), 0).float())
        sa.attn.in_proj_bias.copy_(torch.cat((inp["bqk"], inp["bv"]), 0).float())
        for n in (n1, n2, n3, dec.norm):
            n.eps = inp["eps"]
    return dec.to(device).to(inp["dtype"]).eval(), reg.to(device).to(inp["dtype"]).eval()


def pack(inp, device="cpu"):
    """-> dict(tail, head, pos, fin): the four blobs.  On a device through DinoTransformerDecoder._fused_weights (every check
    of the product's route included: it must accept the module); on the CPU, where that route declines every module, through
    the method it packs with"""
    dec, reg = build_module(inp, device)
    if torch.device(device).type == "cuda":
        blobs = dec._fused_weights(reg)
        assert blobs is not None, "DinoTransformerDecoder._fused_weights declined the module"
        assert (blobs["L"], blobs["P"], blobs["F"]) == (inp["L"], inp["P"], F)
    else:
        blobs = dec._pack_blobs(reg, inp["L"], inp["P"], F)
    return dict(tail=blobs["tails"][0], head=blobs["heads"][0], pos=blobs["pos"], fin=blobs["fin"])


def _unfrag(flat, N, K):
    """the inverse of the fragment-major order: block (tile, ks) at ((tile K / 32 + ks) 64 + lane) 8, lane = 16 g + r, holds
    w[16 tile + r][32 ks + 8 g .. + 7]"""
    w = torch.empty(N, K, dtype=flat.dtype, device=flat.device)
    i = torch.arange(N * K, device=flat.device)
    e, lane, blk = i % 8, (i // 8) % 64, i // 512
    tile, ks = blk // (K // 32), blk % (K // 32)
    w[16 * tile + lane % 16, 32 * ks + 8 * (lane // 16) + e] = flat
    return w


def unpack(blobs, L, P):
    """the documented layout read back -> the weights under the names of weight_shapes (padding rows must be zero)"""
    n_off, n_log = M * L * P * 2, M * L * P
    out, t, o = {}, blobs["tail"], 0

    def mat(src, o, N, K):
        return _unfrag(src[o:o + N * K], N, K), o + N * K

    out["wo"], o = mat(t, o, C, C)
    wol, o = mat(t, o, 512, C)
    out["woff"], out["wlog"] = wol[:n_off], wol[n_off:n_off + n_log]
    assert not bool(wol[n_off + n_log:].any()), "padding rows of the (offsets | logits) matrix are not zero"
    out["wout"], o = mat(t, o, C, C)
    out["w1"], o = mat(t, o, F, C)
    out["w2"], o = mat(t, o, C, F)
    out["wr1"], o = mat(t, o, C, C)
    out["wr2"], o = mat(t, o, C, C)
    wr3, o = mat(t, o, 16, C)
    out["wr3"] = wr3[:4]
    assert not bool(wr3[4:].any())
    for k, n in (("bo", C), ("g1", C), ("e1", C), ("boff", n_off), ("blog", n_log), ("bout", C), ("g2", C), ("e2", C), ("b1", F),
                 ("b2", C), ("g3", C), ("e3", C), ("br1", C), ("br2", C), ("br3", 4)):
        out[k], o = t[o:o + n], o + n
    assert o + 4 == t.numel() and not bool(t[o:].any())
    hd = blobs["head"]
    out["wqk"], o = mat(hd, 0, 2 * C, C)
    out["wv"], o = mat(hd, o, C, C)
    out["bqk"], out["bv"] = hd[o:o + 2 * C], hd[o + 2 * C:]
    ps = blobs["pos"]
    out["wp1"], o = mat(ps, 0, C, 2 * C)
    out["wp2"], o = mat(ps, o, C, C)
    out["bp1"], out["bp2"] = ps[o:o + C], ps[o + C:]
    out["gf"], out["ef"] = blobs["fin"][:C], blobs["fin"][C:]
    return out


# ------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def to_device(inp, device):
    return {k: v.to(device) if torch.is_tensor(v) else v for k, v in inp.items()}


def _blank(dt, L, P, B, Nq, tail=True, head=True):
    """every weight zero, the norms' gamma 1, the activations zero, every valid ratio 1"""
    shapes = PYRAMID[:L]
    _, S = level_starts(shapes)
    rows = B * Nq
    inp = dict(dtype=dt, L=L, P=P, shapes=shapes, B=B, Nq=Nq, tail=tail, head=head, eps=1e-5, temperature=10000.0)
    for k, shp in weight_shapes(L, P).items():
        inp[k] = torch.ones(shp) if k in ("g1", "g2", "g3", "gf") else torch.zeros(shp)
    inp.update(x=torch.zeros(rows, C), attn=torch.zeros(rows, C), qpos=torch.zeros(rows, C), ref=torch.zeros(rows, 4),
               vr32=torch.ones(B, L, 2), value=torch.zeros(B, S, M, D))
    return inp


def _finish(inp):
    dt = inp["dtype"]
    out = {}
    for k, v in inp.items():
        out[k] = v.to(dt) if torch.is_tensor(v) and k != "vr32" else v
    out["vr32"] = inp["vr32"].float()
    return out


def _ri(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).float()


def _affine(g, n=C):
    return 1 + 0.1 * torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)


def value_pattern(B, S):
    """integers 0 .. 7 that differ per pixel, head, channel and image (an odd multiple of the pixel index per channel, so that
    neighbouring pixels differ in every channel); head 7 is zero: its channels anchor the scale and the shift of LN2"""
    b, s = torch.arange(B).view(B, 1, 1, 1), torch.arange(S).view(1, S, 1, 1)
    m, c = torch.arange(M).view(1, 1, M, 1), torch.arange(D).view(1, 1, 1, D)
    v = (s * (2 * (c % 4) + 1) + 3 * c + 5 * m + 3 * b + (s // 3) * (c // 4)) % 8
    v = v.float()
    v[:, :, M - 1] = 0.0
    return v


# candidate offsets: every multiple of 1/4 up to 32 in size is a value of both types
_CAND = torch.arange(-128, 129).double() / 4
PIXEL, HALF, QUARTER, EDGE, FAR = 1, 2, 3, 4, 5


def _classify(im, size):
    """the category of a sample coordinate im (float64, a multiple of 1/4 where > 0) on an axis of `size` pixels"""
    code = torch.zeros_like(im, dtype=torch.long)
    quarter = (im * 4) == (im * 4).round()
    inside = (im >= 0) & (im <= size - 1)
    code = torch.where(quarter & inside, torch.full_like(code, QUARTER), code)
    code = torch.where(quarter & inside & ((im * 2) == (im * 2).round()), torch.full_like(code, HALF), code)
    code = torch.where(quarter & inside & (im == im.round()), torch.full_like(code, PIXEL), code)
    edge = (im == -1) | (im == -0.5) | (im == size - 1) | (im == size - 0.5) | (im == size)
    code = torch.where(edge, torch.full_like(code, EDGE), code)
    code = torch.where(quarter & ((im <= -2) | (im >= size + 1)), torch.full_like(code, FAR), code)
    return code


def gather_exact(dt, L, P, B=3, Nq=37, seed=0):
    """every sample of the gather lands on a multiple of a quarter pixel, every attention weight is 1, 1/2, 1/4 (or 1/16 over all
    points at L P = 16) and the value map holds the integers 0 .. 7: s is exact in fp32 in any order and a value of both types"""
    g = _gen(100 * L + P + seed)
    LP, rows = L * P, B * Nq
    assert rows <= C
    inp = _blank(dt, L, P, B, Nq)
    inp["g1"] = torch.zeros(C)                                     # x1 = 0, q2 = qpos
    inp["x"] = _ri(g, -3, 3, rows, C)
    inp["qpos"] = torch.eye(C)[:rows]                              # row r reads column r of Wol: its own table
    inp["ref"] = 30.0 * torch.randint(0, 2, (rows, 4), generator=g).float()
    ratios = torch.tensor([0.5, 0.75, 1.0])
    inp["vr32"] = ratios[torch.randint(0, 3, (B, L, 2), generator=g)]
    for b in range(B):                                             # differ per image and level, and level 0 from the others
        for l in range(L):
            inp["vr32"][b, l, 0] = ratios[(b + l) % 3]
            inp["vr32"][b, l, 1] = ratios[(2 * b + l + 1) % 3]
    _, S = level_starts(inp["shapes"])
    inp["value"] = value_pattern(B, S)
    # ---- positions: for every (row, level, axis) the sample coordinate of every candidate offset, in float64 (exact)
    sig = torch.where(inp["ref"] > 0, 1.0, 0.5).double()          # [rows, 4]
    bidx = torch.arange(rows) // Nq
    lvl = torch.arange(LP) // P
    size = torch.tensor([[w, h] for h, w in inp["shapes"]]).double()[lvl]            # [LP, 2] (x, y)
    vr = inp["vr32"].double()[bidx][:, lvl]                                           # [rows, LP, 2]
    centre, extent = sig[:, None, :2] * vr, sig[:, None, 2:] * vr                     # [rows, LP, 2]
    im = (_CAND.view(1, 1, 1, -1) * (extent * (0.5 / P))[..., None] + centre[..., None]) * size[None, :, :, None] - 0.5
    code = _classify(im, size[None, :, :, None])                                      # [rows, LP, 2, cand]
    ok_any = code > 0                                                                 # a multiple of a quarter pixel
    ok_int = ok_any & ((im == im.round()) | (code == FAR))                            # ... whose bilinear weights are 0 or 1
    feas1, feasN = ok_any.any(-1).all(-1), ok_int.any(-1).all(-1)                     # [rows, LP]
    # ---- attention: which points of a (row, head) carry weight.  A point whose box admits no such offset carries none
    mode = torch.randint(0, 4 if LP == 16 else 3, (rows, M), generator=g)   # 0: one point, 1: two, 2: four, 3: all sixteen
    rank = (torch.rand(rows, M, LP, generator=g) + 2.0 * ~feasN[:, None]).argsort(-1).argsort(-1)
    sel = torch.zeros(rows, M, LP, dtype=torch.bool)
    for n, k in ((1, 2), (2, 4), (3, 16)):
        sel |= ((mode == n) & (feasN.sum(-1)[:, None] >= k))[..., None] & (rank < k)
    first = (torch.arange(rows)[:, None] + 3 * torch.arange(M)[None]) % LP   # every point is the single one of some row
    walk = (first[..., None] + torch.arange(LP)) % LP                                 # the first point from there that can be
    can = feas1[torch.arange(rows)[:, None, None], walk]
    assert bool(can.any(-1).all()), "a row admits no exact sample at all"
    first = torch.gather(walk, -1, can.float().argmax(-1, keepdim=True))[..., 0]
    one = sel.sum(-1) == 0
    sel = torch.where(one[..., None], torch.arange(LP)[None, None] == first[..., None], sel)
    single = sel.sum(-1, keepdim=True) == 1
    want = torch.randint(1, 6, (rows, M, LP, 2), generator=g)
    # fractional bilinear weights only under an attention weight of 1 (the sum stays within 8 significant bits)
    whole = (want == PIXEL) | (want == FAR) | (want == EDGE)
    want = torch.where(single[..., None] | whole, want, torch.full_like(want, PIXEL))
    c = code[:, None]                                                                 # [rows, 1, LP, 2, cand]
    allowed = torch.where(single[..., None, None], ok_any[:, None], ok_int[:, None])
    allowed = allowed | ~sel[..., None, None]                                         # a point of weight 0 may lie anywhere
    score = torch.rand(rows, M, LP, 2, _CAND.numel(), generator=g) + 4.0 * (c == want[..., None]) + 8.0 * allowed
    pick = score.argmax(-1)                                                           # [rows, M, LP, 2]
    assert bool(torch.gather(allowed, -1, pick[..., None]).all()), "no exact offset for a sample"
    off = _CAND[pick].float()                                                         # [rows, M, LP, 2]
    logit = torch.where(sel, 0.0, -30000.0)
    inp["woff"] = torch.zeros(M * LP * 2, C)
    inp["woff"][:, :rows] = off.reshape(rows, -1).t()
    inp["wlog"] = torch.zeros(M * LP, C)
    inp["wlog"][:, :rows] = logit.reshape(rows, -1).t()
    # ---- a signed permutation out of the gather; the channels fed by the zero head carry a fixed integer pattern
    perm = torch.randperm(C, generator=g)
    sign = 1.0 - 2.0 * torch.randint(0, 2, (C,), generator=g)
    inp["wout"] = torch.zeros(C, C)
    inp["wout"][torch.arange(C), perm] = sign
    n = torch.arange(C)
    inp["bout"] = torch.where(perm // D == M - 1, ((n % 5) + 1.0) * (1.0 - 2.0 * (n % 2)), torch.zeros(C))
    return _finish(inp)


def oproj_exact(dt, L=5, P=4, B=3, Nq=37, seed=0):
    """Wo attn + bo are integers just below and above the largest one the type counts to, so E moves the odd ones above it; x
    brings the sum back to 128 +- 10: t1 is an exact integer whichever way E went, and rows of a mean far above their spread"""
    g = _gen(7 + seed)
    rows, lim = B * Nq, INT_LIMIT[dt]
    inp = _blank(dt, L, P, B, Nq)
    inp["attn"] = _ri(g, -2, 2, rows, C)
    inp["wo"] = fb._sparse_pm1(C, C, 4, g)
    inp["bo"] = torch.full((C,), float(lim))
    inp["x"] = -(lim - 128.0) + _ri(g, -2, 2, rows, C)
    inp["qpos"] = _ri(g, -2, 2, rows, C)
    for k in ("1", "2", "3"):
        inp["g" + k], inp["e" + k] = _affine(g)
    inp["ref"] = _ri(g, -8, 8, rows, 4) / 4
    _, S = level_starts(inp["shapes"])
    inp["value"] = value_pattern(B, S)
    return _finish(inp)


def ffn_exact(dt, L=5, P=4, B=3, Nq=307, seed=0):
    """x2 = beta2, integers, in every row; sparse +-1 W1 / W2 and a b1 that differs between the chunks at every column and
    between the columns: every row has the same integer y32, whichever order its workgroup walks the chunks in"""
    g = _gen(11 + seed)
    rows = B * Nq
    inp = _blank(dt, L, P, B, Nq)
    inp["x"] = _ri(g, -3, 3, rows, C)
    inp["g2"], inp["e2"] = torch.zeros(C), _ri(g, -3, 3, C)
    inp["w1"] = fb._sparse_pm1(F, C, 4, g)
    j = torch.arange(F)
    inp["b1"] = ((5 * (j // 256) + 3 * (j % 256)) % 16 - 6).float()
    inp["w2"] = fb._sparse_pm1(C, F, 3, g)
    inp["b2"] = _ri(g, -2, 2, C)
    return _finish(inp)


def ffn_rounding(dt, L=5, P=4, B=3, Nq=37, seed=0):
    """x2 = 4096 in every channel; balanced W1 rows leave h = relu(b1), two hidden units per output channel 0 .. 31 are
    8192 + 3 (which E moves to 8192) and 8192, and W2 takes their difference: y32 = 4096 + small integers, exact in fp32 and
    not values of either type.  Catches a hidden activation kept in fp32, a y32 that is rounded, a one-pass variance"""
    g = _gen(13 + seed)
    rows = B * Nq
    inp = _blank(dt, L, P, B, Nq)
    inp["x"] = _ri(g, -3, 3, rows, C)
    inp["g2"], inp["e2"] = torch.zeros(C), torch.full((C,), 4096.0)
    w1 = torch.zeros(F, C)
    idx = torch.rand(F, C, generator=g).argsort(1)[:, :4]
    w1.scatter_(1, idx, torch.tensor([1.0, 1.0, -1.0, -1.0]).expand(F, 4).contiguous())
    inp["w1"] = w1
    inp["b1"] = _ri(g, -4, 6, F)
    w2 = fb._sparse_pm1(C, F, 3, g)
    for n in range(32):                                    # hidden units 64 n (+ 3) and 64 n + 1 (+ 0), both 2 x 4096 + b1
        for k, b1 in ((64 * n, 3.0), (64 * n + 1, 0.0)):
            inp["w1"][k] = 0.0
            inp["w1"][k, n] = inp["w1"][k, n + 32] = 1.0
            inp["b1"][k] = b1
            w2[:, k] = 0.0
        w2[n, 64 * n], w2[n, 64 * n + 1] = 1.0, -1.0
    inp["w2"] = w2
    inp["b2"] = _ri(g, -2, 2, C)
    return _finish(inp)


def box_exact(dt, L=5, P=4, B=3, Nq=37, seed=0, head=True):
    """x3 = beta3, integers; integer reg branch, in-projection of v and output norm; coordinate 3 of the box delta is the first
    odd integer above the type's exact ones, so E moves it before the reference point is added"""
    g = _gen(17 + seed)
    rows, lim = B * Nq, INT_LIMIT[dt]
    inp = _blank(dt, L, P, B, Nq, head=head)
    inp["x"], inp["attn"] = _ri(g, -3, 3, rows, C), _ri(g, -2, 2, rows, C)
    inp["wo"] = fb._sparse_pm1(C, C, 4, g)
    inp["g3"], inp["e3"] = torch.zeros(C), _ri(g, -3, 3, C)
    inp["wr1"], inp["br1"] = fb._sparse_pm1(C, C, 4, g), _ri(g, -2, 2, C)
    inp["wr2"], inp["br2"] = fb._sparse_pm1(C, C, 4, g), _ri(g, -2, 2, C)
    inp["wr2"][0], inp["br2"][0] = 0.0, 1.0                # r2[0] = 1
    wr3 = fb._sparse_pm1(4, C, 4, g)
    wr3[:, 0] = 0.0
    wr3[3] = 0.0
    wr3[3, 0] = 1.0
    inp["wr3"], inp["br3"] = wr3, torch.tensor([1.0, -2.0, 0.0, float(lim)])
    ref = _ri(g, -16, 16, rows, 4) / 8 + (torch.arange(rows) % 8).view(-1, 1) / 8
    ref[:, 3] = -(lim - 8.0) + (torch.arange(rows) % 4).float()
    inp["ref"] = ref
    inp["wv"], inp["bv"] = fb._sparse_pm1(C, C, 4, g), _ri(g, -2, 2, C)
    inp["gf"], inp["ef"] = torch.zeros(C), ((torch.arange(C) % 7) - 3.0)
    inp["vr32"] = 0.5 + 0.5 * torch.rand(B, L, 2, generator=g)
    inp["bp2"] = _ri(g, -2, 2, C)                          # qpos' = bp2: a v taken from x3 + qpos' shows
    return _finish(inp)


SINE_SELECTIONS = 4


def sine_exact(dt, sel, L=5, P=4, B=3, Nq=37, seed=0):
    """HEAD-only: qpos_out[n] = relu(E(sine[128 sel + n])), qpos_out[128 + n] = relu(-E(sine[128 sel + n])) for n < 128"""
    g = _gen(19 + seed)
    rows = B * Nq
    inp = _blank(dt, L, P, B, Nq, tail=False)
    n = torch.arange(128)
    inp["wp1"][n, 128 * sel + n] = 1.0
    inp["wp1"][128 + n, 128 * sel + n] = -1.0
    inp["wp2"] = torch.eye(C)
    inp["ref"] = 2.0 * torch.randn(rows, 4, generator=g)
    inp["ref"][0] = torch.tensor([20.0, -20.0, 0.0, 8.0])
    vr = 0.5 + 0.25 * torch.rand(B, L, 2, generator=g)
    vr[:, 0] = 0.8 + 0.2 * torch.rand(B, 2, generator=g)          # level 0 is not the other levels
    inp["vr32"] = vr
    inp["x"] = _ri(g, -3, 3, rows, C)
    return _finish(inp)


def sine_error(qpos_out, ex, sel):
    """largest |E(sine) read back from qpos_out - float64 sine| over the 128 channels of selection `sel`"""
    got = qpos_out.double()
    back = got[:, :128] - got[:, 128:]
    return float((back - ex.stages["sine64"][:, 128 * sel:128 * (sel + 1)]).abs().max())


def sine_allowance(dt):
    """the project's allowance for this embedding (tests/test_bf16_kernels_gpu.py: one rounding of a value in [-1, 1] and the
    fast-path sin / cos)"""
    return U[dt] + 1e-3


def random_layer(dt, L, P, B=3, Nq=37, seed=0, head=True):
    """trained-like scales (tests/test_decoder_layer_gpu.py's _decoder); offsets that reach beyond the image; 10 % of the value
    rows masked"""
    g = _gen(1000 * L + 10 * P + seed)
    rows = B * Nq
    inp = _blank(dt, L, P, B, Nq, head=head)
    for k, shp in weight_shapes(L, P).items():
        if len(shp) == 2:
            inp[k] = torch.randn(shp, generator=g) * (1.0 / shp[1]) ** 0.5
        else:
            inp[k] = torch.randn(shp, generator=g) * 0.1
    for k in ("g1", "g2", "g3", "gf"):
        inp[k] = inp[k] + 1.0
    inp["woff"] = inp["woff"] * 0.5
    inp["boff"] = torch.randn(inp["boff"].shape, generator=g) * 2.0
    inp["wr3"] = inp["wr3"] * 0.2
    _, S = level_starts(inp["shapes"])
    inp["x"], inp["attn"] = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    inp["qpos"] = torch.randn(rows, C, generator=g)
    inp["ref"] = torch.randn(rows, 4, generator=g) * 1.5
    inp["vr32"] = 0.6 + 0.4 * torch.rand(B, L, 2, generator=g)
    value = torch.randn(B, S, M, D, generator=g)
    value[torch.rand(B, S, generator=g) < 0.1] = 0.0
    inp["value"] = value
    return _finish(inp)


def rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-30))


def outputs_of(inp):
    """the names of the outputs the launch form of `inp` writes"""
    return (("x_out", "ref_out") if inp["tail"] else ()) + (("qpos_out", "qk_out", "v_out") if inp["head"] else ())


# ------------------------------------------------------------------------------------------------------- cases
def _lp(L, P):
    return f"L{L}P{P}"


def case_names():
    names = [f"gather_exact_{_lp(L, P)}" for L, P in LP_PROBES] + ["oproj_exact", "ffn_exact", "ffn_rounding", "box_exact_head",
                                                                  "box_exact_tail", "sine_exact"]
    return names + [f"random_{_lp(L, P)}_{form}" for L, P in LP_RANDOM for form in ("head", "tail")]


CASE_NAMES = tuple(case_names())
BOUND_CASES = tuple(n for n in CASE_NAMES if n.startswith(("gather_exact", "oproj_exact", "ffn_exact", "ffn_rounding")))


def build(name, dt):
    """the inputs of a case on the CPU (sine_exact: a list of the four selections)"""
    rest = name.partition("_L")[2]
    if name.startswith("gather_exact"):
        L, P = (int(v) for v in rest.split("P"))
        return gather_exact(dt, L, P)
    if name.startswith("random"):
        lp, form = rest.split("_")
        L, P = (int(v) for v in lp.split("P"))
        return random_layer(dt, L, P, head=form == "head")
    if name == "sine_exact":
        return [sine_exact(dt, sel) for sel in range(SINE_SELECTIONS)]
    return {"oproj_exact": oproj_exact, "ffn_exact": ffn_exact, "ffn_rounding": ffn_rounding,
            "box_exact_head": lambda d: box_exact(d, head=True), "box_exact_tail": lambda d: box_exact(d, head=False)}[name](dt)


def _same(got, want, what):
    assert got.shape == want.shape and bool(torch.isfinite(got.float()).all()), what
    bad = int((got.double() != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.numel()} elements are not the exact value"


def hold(name, dt, run, device="cpu"):
    """run(inp) -> Outputs on one case; raises AssertionError where the case's criterion fails, returns the measured figures"""
    import helpers_model as hm

    built = build(name, dt)
    fig = {}
    if name == "sine_exact":
        worst = 0.0
        for sel, inp in enumerate(built):
            inp = to_device(inp, device)
            ex, out = exact(inp), run(inp)
            assert out.qpos_out.dtype == dt and bool(torch.isfinite(out.qpos_out.float()).all())
            assert bool((out.qpos_out[:, :128].float() * out.qpos_out[:, 128:].float() == 0).all()), "relu(+s) and relu(-s) both set"
            worst = max(worst, sine_error(out.qpos_out, ex, sel))
        fig["sine_err"] = worst
        fig["allowance"] = sine_allowance(dt)
        assert worst <= sine_allowance(dt), f"{name}: sine error {worst:.3e} > {sine_allowance(dt):.3e}"
        return fig
    inp = to_device(built, device)
    ex, out = exact(inp), run(inp)
    for k in outputs_of(inp):
        assert getattr(out, k).dtype == dt and getattr(out, k).shape == getattr(ex, k).shape, k
    if name in BOUND_CASES:
        b = bound(ex)
        assert bool(torch.isfinite(b).all()), f"{name}: the bound is not finite for every element"
        fig["ratio"] = ratio(out.x_out, ex.x_out, b)
        if name == "ffn_exact":
            rows_same = bool((out.x_out.double() == out.x_out[0].double()).all())
            fig["rows_identical"] = rows_same
            assert rows_same, f"{name}: a row of x_out differs from row 0"
        assert fig["ratio"] <= 1.0, f"{name}: err / bound {fig['ratio']:.3g}"
    elif name.startswith("box_exact"):
        _same(out.ref_out, ex.ref_out, name + " ref_out")
        if inp["head"]:
            _same(out.v_out, ex.v_out, name + " v_out")
        else:
            _same(out.x_out, ex.x_out, name + " x_out")
        fig["bit_exact"] = True
    else:                                        # random
        scale = 1.0 if dt == torch.float16 else 8.0
        emu = emulate(inp)
        for k in outputs_of(inp):
            got, want = getattr(out, k), getattr(ex, k)
            e_k, e_e = rel_l2(got, want), rel_l2(getattr(emu, k), want)
            fig[k] = (e_k, e_e)
        for k in outputs_of(inp):
            got, want = getattr(out, k), getattr(ex, k)
            hm.assert_rows_close(got.double().cpu().numpy(), want.cpu().numpy(), 3e-3 * scale, what=f"{name} {k}")
            e_k, e_e = fig[k]
            assert e_k <= 1.5 * e_e + 1e-3 * scale, f"{name} {k}: rel-L2 {e_k:.3e} against the emulation's {e_e:.3e}"
    return fig


def run_kernel(inp, blobs=None, guard=0, sentinel=-7.0):
    """one launch of codetr_decoder_layer_{f16,bf16} on the device tensors of `inp` -> Outputs [rows + guard, ...]: every output
    is allocated with `guard` extra rows of `sentinel` behind `rows`, every input exactly `rows` long"""
    from codetr import _cabi

    dev, dt = inp["x"].device, inp["dtype"]
    blobs = pack(inp, dev) if blobs is None else blobs
    B, Nq, L, P = inp["B"], inp["Nq"], inp["L"], inp["P"]
    rows = B * Nq
    starts, S = level_starts(inp["shapes"])
    ss = torch.tensor(inp["shapes"], dtype=torch.int64, device=dev)
    ls = torch.tensor(starts, dtype=torch.int64, device=dev)
    new = lambda w: torch.full((rows + guard, w), sentinel, dtype=dt, device=dev)   # noqa: E731
    tail, head = inp["tail"], inp["head"]
    x_out, ref_out = (new(C), new(4)) if tail else (None, None)
    qpos_out, qk_out, v_out = (new(C), new(2 * C), new(C)) if head else (None, None, None)
    cg = lambda k: inp[k].contiguous()   # noqa: E731
    assert inp["x"].shape[0] == rows and inp["ref"].shape[0] == rows
    with torch.cuda.device(dev):
        _cabi.decoder_layer(cg("x"), cg("attn") if tail else None, cg("qpos") if tail else None, cg("ref"), cg("vr32"),
                            cg("value") if tail else None, ss if tail else None, ls if tail else None,
                            blobs["tail"] if tail else None, blobs["pos"] if head else None, blobs["head"] if head else None,
                            blobs["fin"] if tail and not head else None, x_out, ref_out, qpos_out, qk_out, v_out,
                            B, Nq, S, L, P, F, inp["eps"], inp["temperature"])
        torch.cuda.synchronize(dev)
    return Outputs(x_out, ref_out, qpos_out, qk_out, v_out)


def valid_rows(out, rows):
    return Outputs(*[None if t is None else t[:rows] for t in out])
