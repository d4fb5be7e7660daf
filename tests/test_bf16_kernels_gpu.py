"""The 16-bit head / decoder / geometry kernels in bf16 (and the fp32 twins of the fp16 route) against plain float64
evaluations of the same operations on the same 16-bit inputs:
  csrc/small_ops.hip         add (plain, broadcast), sigmoid, gather_rows, valid_ratios (+ out32), decode_boxes
  csrc/encoder_geometry.hip  reference points, per-level points, proposals, keep / drop state; row_max
  csrc/query_sine_embed.hip  ref_in, the sine embedding, and ref_in32 when valid_ratios carries its fp32 twin

Bounds are derived from where each kernel rounds.  u is the unit roundoff of the storage type (fp16 2^-11, bf16 2^-8):
one round-to-nearest of a normal value x errs by at most u |x| (one ulp is at most 2u |x|).  Arithmetic between
roundings runs in fp32 (unit roundoff 2^-24); where that can matter the fp32 term is written out next to u."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
U32 = 2.0 ** -24
# smallest positive normal of the storage type: below it round-to-nearest errs by half the subnormal step instead
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
DT = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _g(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _within(got, exact, rel, absolute=0.0):
    """|got - exact| <= rel |exact| + absolute everywhere, NaN exactly where exact is NaN"""
    got, exact = got.double(), exact.double()
    assert torch.equal(got.isnan(), exact.isnan()), "NaN pattern differs"
    fin = ~exact.isnan()
    err = (got[fin] - exact[fin]).abs()
    lim = rel * exact[fin].abs() + absolute
    bad = err > lim
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} elements outside the bound; worst excess "
                           f"{float((err - lim).max()):.3e}, e.g. got {float(got[fin][bad][0])} exact {float(exact[fin][bad][0])}")


# ---- small ops (csrc/small_ops.hip) ----------------------------------------------------------------------------------

def test_add_bf16_plain_and_broadcast():
    """ATen's bf16 add computes in fp32 and rounds once: bit-identical.  Against float64: the fp32 sum (<= U32) then the
    bf16 rounding (<= u)."""
    from codetr import _cabi, hip_ops

    dt, g = torch.bfloat16, _g(10)
    a = (torch.randn(3, 900, 256, device=DEV, generator=g) * 4).to(dt)
    b = torch.randn(3, 900, 256, device=DEV, generator=g).to(dt)
    w = torch.randn(900, 256, device=DEV, generator=g).to(dt)
    before = _cabi.CALLS["small_ops"]
    plain, bcast = hip_ops.add(a, b), hip_ops.add(w[None].expand(3, -1, -1), b)
    assert _cabi.CALLS["small_ops"] == before + 2
    assert plain.dtype == bcast.dtype == dt
    assert torch.equal(plain, a + b) and torch.equal(bcast, w[None] + b)
    _within(plain, a.double() + b.double(), U[dt] + U32, 1e-38)
    _within(bcast, w[None].double() + b.double(), U[dt] + U32, 1e-38)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_sigmoid_against_float64(dtype):
    """fp32 sigmoid (expf within a few fp32 ulps; the sigmoid's condition number w.r.t. exp is <= 1) rounded once:
    <= u + 2^-21 relative, plus half the subnormal step for fp16's tiny outputs"""
    from codetr import hip_ops

    x = (torch.randn(2, 900, 80, device=DEV, generator=_g(11)) * 4).to(dtype)
    x[0, 0, :8] = torch.tensor([0.0, -30.0, 30.0, float("nan"), float("inf"), -float("inf"), -0.0, 88.0],
                               device=DEV).to(dtype)
    got = hip_ops.sigmoid(x)
    assert got.dtype == dtype
    _within(got, torch.sigmoid(x.double()), U[dtype] + 2.0 ** -21, TINY[dtype])
    ref = x.sigmoid()    # ATen: fp32 sigmoid rounded once; the two fp32 exps may differ in their last bit
    same = (got == ref) | (got.isnan() & ref.isnan())
    assert same.float().mean() > 0.999


@pytest.mark.parametrize("C", [256, 4])
def test_gather_rows_bf16(C):
    """a copy: bit-exact, including the first and the last row of the source"""
    from codetr import hip_ops

    g = _g(12 + C)
    S = 5000
    src = torch.randn(2, S, C, device=DEV, generator=g).to(torch.bfloat16)
    src[0, 0, 0], src[1, S - 1, C - 1] = float("nan"), -0.0
    idx = torch.randint(0, S, (2, 900), device=DEV, generator=g)
    idx[:, 0], idx[:, -1] = 0, S - 1
    out = hip_ops.gather_rows(src, idx)
    ref = torch.gather(src, 1, idx[..., None].expand(-1, -1, C))
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_valid_ratios_and_fp32_twin(dtype):
    """out = round(round(counts) / wh): bit-identical to `counts.to(dtype) / wh` (ATen divides in fp32, rounds once) and,
    against the float64 quotient of the same rounded operands, <= u + U32 (fp32 division, then the storage rounding).
    out32 = counts / wh in fp32, unrounded: <= U32 from float64."""
    from codetr import hip_ops

    g = _g(13)
    counts = torch.randint(1, 480, (3, 5, 2), device=DEV, generator=g).float()
    counts[0, 0] = torch.tensor([479.0, 167.0], device=DEV)      # 9 / 8 significant bits: bf16 rounds them
    wh = torch.tensor([[480.0, 320], [240, 160], [120, 80], [60, 40], [30, 20]], device=DEV).to(dtype)
    wh[0] = torch.tensor([167.0, 100.0])                          # 1333 x 800 / 8: 167 is not a bf16 value
    out = hip_ops.valid_ratios(counts, wh)
    assert out.dtype == dtype and torch.equal(out, counts.to(dtype) / wh)
    _within(out, counts.to(dtype).double() / wh.double(), U[dtype] + U32)
    out32 = getattr(out, "_codetr_f32", None)
    assert out32 is not None and out32.dtype == torch.float32
    _within(out32, counts.double() / wh.double(), U32)


@pytest.mark.parametrize("W,H", [(1920, 1280), (1333, 800)])
def test_decode_boxes_bf16(W, H):
    """Rounding points of the kernel (the ATen bf16 sequence's): sigmoid (u), c -+ w/2 (u), x round(W) (u); W and H
    are rounded to bf16 first, as the ATen scale tensor is (1333 -> 1336).  Against the float64 decode with the rounded
    scale, an output coordinate errs by at most u * scale * (|c| + |w/2| + 2 |c -+ w/2|) (clamping is 1-Lipschitz)."""
    from codetr import hip_ops
    from codetr.co_dino_head import bbox_cxcywh_to_xyxy
    from helpers_model import decode64

    dt, g = torch.bfloat16, _g(14)
    B, Nq, C, K = 2, 900, 80, 300
    unact = (torch.randn(B, Nq, 4, device=DEV, generator=g) * 3).to(dt)
    unact[0, 0] = torch.tensor([20.0, -20.0, 20.0, 20.0])         # saturated: every clamp engages
    unact[0, 1] = torch.tensor([-20.0, 20.0, -20.0, -20.0])
    unact[1, 5, 2] = float("nan")
    idx = torch.randint(0, Nq * C, (B, K), device=DEV, generator=g)
    idx[0, :5] = torch.tensor([0 * C + 3, 1 * C + 0, 1 * C - 1, 0, C])   # class boundaries: labels 0 and C-1
    idx[1, :3] = torch.tensor([5 * C + 7, Nq * C - 1, 5 * C])
    boxes, labels = hip_ops.decode_boxes(unact, idx, C, W, H)
    assert boxes.dtype == dt and torch.equal(labels, idx % C)
    sw, sh = float(torch.tensor(float(W)).to(dt)), float(torch.tensor(float(H)).to(dt))
    exact, mag = decode64(unact, idx, C, sw, sh)
    fin = ~exact.isnan()
    assert torch.equal(boxes.isnan(), exact.isnan())
    err = (boxes.double() - exact).abs()[fin]
    assert (err <= U[dt] * (1 + 4 * U[dt]) * mag[fin] + 1e-30).all(), float((err - U[dt] * mag[fin]).max())
    # the saturated rows: x1 = 0.5 W, y2 = 0.5 H, x2 = W (the rounded W: the clamp bound is the scale tensor itself)
    assert boxes[0, 0].tolist() == [0.5 * sw, 0.0, sw, 0.5 * sh]
    # ATen bf16 sequence on the same inputs: same rounding points; fp32 sigmoid's last bit may differ
    ref = bbox_cxcywh_to_xyxy(torch.gather(unact.sigmoid(), 1, (idx // C)[..., None].expand(-1, -1, 4)))
    scale = ref.new_tensor([W, H, W, H])
    ref = torch.minimum((ref * scale).clamp(min=0), scale)
    both_nan = boxes.isnan() & ref.isnan()
    diff = (boxes != ref) & ~both_nan
    assert diff.float().mean() < 2e-3 and torch.equal(boxes.isnan(), ref.isnan())


# ---- encoder geometry (csrc/encoder_geometry.hip) --------------------------------------------------------------------

def _masks(B, shapes, pad, seed=1):
    g = _g(seed)
    ms = []
    for h, w in shapes:
        m = torch.zeros(B, h, w, dtype=torch.bool, device=DEV)
        if pad:
            for b in range(B):
                m[b, int(h * (0.6 + 0.4 * torch.rand((), device=DEV, generator=g))):, :] = True
                m[b, :, int(w * (0.5 + 0.5 * torch.rand((), device=DEV, generator=g))):] = True
        ms.append(m)
    return ms


def _centres_over_extent(vr, shapes, dtype):
    """float64 (x + 0.5) / round(vr_w W), (y + 0.5) / round(vr_h H) -> [B, S, 2]: exact pixel centres over the valid
    extent, the extent rounded to the storage type as the kernel (and the reference) round it; vr * W is exact in fp32"""
    B = vr.shape[0]
    out = []
    for lvl, (h, w) in enumerate(shapes):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=DEV) + 0.5,
                                torch.arange(w, dtype=torch.float64, device=DEV) + 0.5, indexing="ij")
        dx = (vr[:, lvl, 0].double() * w).to(dtype).double().view(B, 1)
        dy = (vr[:, lvl, 1].double() * h).to(dtype).double().view(B, 1)
        out.append(torch.stack((xs.reshape(1, -1) / dx, ys.reshape(1, -1) / dy), -1))
    return torch.cat(out, 1)


PYRAMIDS = [
    (1, [(160, 240), (80, 120), (40, 60), (20, 30), (10, 15)], False),    # 1920 x 1280
    (2, [(160, 240), (80, 120), (40, 60), (20, 30), (10, 15)], True),
    (2, [(76, 76), (38, 38), (19, 19), (10, 10), (5, 5)], True),
    (3, [(42, 65), (21, 33), (11, 17), (6, 9), (3, 5)], True),
    (1, [(100, 300), (50, 150), (25, 75), (13, 38), (7, 19)], False),     # level-0 width >= 256
    (2, [(100, 300), (50, 150), (25, 75), (13, 38), (7, 19)], True),
]


@pytest.mark.parametrize("B,shapes,pad", PYRAMIDS)
def test_encoder_geometry_bf16_against_float64(B, shapes, pad):
    """Per token: ref = round(fp32((x + .5) / round(vr W)))  -- exact centre, fp32 quotient, one storage rounding:
    <= u + U32 from the float64 quotient, and bit-equal to the fp32 quotient rounded once;
    ref_lvl = round(ref * vr_k), a product exact in fp32: bit-equal;
    proposals (kept) = round(fp32 logit(ref_x, ref_y, w_l, w_l)), w_l = round(fp32(0.05) 2^l): <= u |L| + 2^-21
    (fp32 division and logf) from the float64 logit of the same inputs; dropped: finfo(bf16).max where the logit is
    finite, NaN where it is not; keep / drop equals the float64 decision except within one bf16 ulp (2^-5) of +-4.6."""
    from codetr import _cabi, hip_ops
    from codetr import transformer as T

    dt = torch.bfloat16
    masks = _masks(B, shapes, pad)
    mask_flat = torch.cat([m.flatten(1) for m in masks], 1)
    vr = torch.stack([T.get_valid_ratio(m, dtype=dt) for m in masks], 1)
    before = _cabi.CALLS["encoder_geometry"]
    ref, ref_lvl, prop, state = hip_ops.encoder_geometry(vr, mask_flat, shapes)
    assert _cabi.CALLS["encoder_geometry"] == before + 1
    assert ref.dtype == ref_lvl.dtype == prop.dtype == dt
    q = _centres_over_extent(vr, shapes, dt)
    _within(ref, q, U[dt] + U32)
    assert torch.equal(ref, q.float().to(dt))
    assert torch.equal(ref_lvl, (ref.float()[:, :, None] * vr.float()[:, None]).to(dt))
    # proposals on the kernel's own (just verified) reference points
    L = len(shapes)
    wl = torch.cat([torch.full((h * w,), float(torch.tensor(0.05 * 2 ** l, dtype=torch.float32).to(dt)),
                               dtype=torch.float64, device=DEV) for l, (h, w) in enumerate(shapes)])
    wl = wl.view(1, -1, 1).expand(B, -1, 2)
    p = torch.cat((ref.double(), wl), -1)
    logit = torch.log(p / (1 - p))
    finite = torch.isfinite(logit)
    inside = ((logit > -4.6) & (logit < 4.6)).all(-1)
    keep = inside & ~mask_flat
    near = (((logit.abs() - 4.6).abs() <= 2.0 ** -5) & finite).any(-1)
    assert set(state.unique().tolist()) <= {0, 2}
    assert torch.equal((state == 0)[~near], keep[~near])
    k = state == 0
    assert L == vr.shape[1] and k.any()
    _within(prop[k], logit[k], U[dt], 2.0 ** -21)
    d, dfin = prop[~k], finite[~k]
    assert (d[dfin] == torch.finfo(dt).max).all() and torch.isnan(d[~dfin]).all()
    if pad:
        assert (~dfin).any(), "a padded pyramid has centres beyond the valid extent: non-finite logits"


@pytest.mark.parametrize("B,shapes,pad", [PYRAMIDS[1], PYRAMIDS[5]])
def test_bf16_exact_centres_are_no_further_from_float64_than_aten(B, shapes, pad):
    """The kernel takes pixel centres exactly ((float)x + .5); the ATen formulation (transformer._pixel_centres,
    torch.linspace in bf16) cannot represent a .5 centre from 128 up.  Per point the native value is the nearest bf16
    value of the quotient (up to the fp32 quotient's own rounding), so it is never further from float64 than ATen's."""
    from codetr import hip_ops
    from codetr import transformer as T

    dt = torch.bfloat16
    masks = _masks(B, shapes, pad, seed=2)
    mask_flat = torch.cat([m.flatten(1) for m in masks], 1)
    vr = torch.stack([T.get_valid_ratio(m, dtype=dt) for m in masks], 1)
    ref = hip_ops.encoder_geometry(vr, mask_flat, shapes)[0]
    aten = T.get_reference_points([tuple(s) for s in shapes], vr, device=DEV)
    q = _centres_over_extent(vr, shapes, dt)
    e_native, e_aten = (ref.double() - q).abs(), (aten.double() - q).abs()
    assert (e_native <= e_aten + 2 * U32 * q.abs()).all()
    assert float(e_native.sum()) < float(e_aten.sum())      # level 0 is wider than 128: ATen's centres are off there


@pytest.mark.parametrize("rows,C", [(204600, 80), (1000, 81), (7, 8), (33, 300)])
def test_row_max_bf16_against_float64(rows, C):
    """a selection: bit-equal to the float64 row max of the same values, NaN wherever a row holds one, -inf for
    all -inf rows"""
    from codetr import hip_ops

    dt, g = torch.bfloat16, _g(15 + C)
    x = torch.randn(rows, C, device=DEV, generator=g).to(dt)
    x[3, C // 2] = float("nan")
    x[4, C - 1] = float("nan")                     # the last column: the tail of the vector loop / of the ragged loop
    x[4, 0] = float("inf")
    x[5] = float("-inf")
    x[6] = float("-inf")
    x[6, C - 1] = float("nan")
    x[2] = -torch.finfo(dt).max
    y = hip_ops.row_max(x)
    ref = x.double().max(-1)[0]
    assert y.dtype == dt and torch.equal(y.isnan(), ref.isnan())
    assert bool(torch.isnan(y[[3, 4, 6]]).all()) and float(y[5]) == -math.inf
    fin = ~ref.isnan()
    assert torch.equal(y.double()[fin], ref[fin])
    x3 = x[:min(rows, 6)].reshape(1, -1, C)        # [B, S, C] views keep their leading shape
    assert torch.equal(hip_ops.row_max(x3).view(torch.int16), hip_ops.row_max(x3.reshape(-1, C)).view(1, -1).view(torch.int16))


# ---- decoder query positions (csrc/query_sine_embed.hip) -------------------------------------------------------------

@pytest.mark.parametrize("with32", [False, True], ids=["16bit", "fp32twin"])
@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("B,Nq,d,L", [(1, 900, 4, 5), (2, 50, 2, 5)])
def test_query_sine_embed_against_float64(B, Nq, d, L, dtype, with32):
    """ref_in = round(round(sigmoid(ref)) * vr): two roundings (the product of two storage values is exact in fp32)
    and __expf's error (<= 2^-19 relative here): <= (2u + u^2 + 2^-19) |exact|, i.e. within one ulp of float64.
    The embedding: sin / cos in fp32 of the same coordinate, rounded once: <= u (values in [-1, 1]) + 1e-3, the
    fast-path sin / cos allowance of the fp16 test (its 1.5e-3 less its own 2^-11 rounding).
    With the fp32 twin of the valid ratios: ref_in32 = sigmoid(ref) * vr32 in fp32 (expf, 1 +, division, product:
    a few fp32 roundings) <= 2^-21 relative, and the embedding is taken from it."""
    from codetr import hip_ops
    from codetr.transformer import DinoTransformerDecoder

    g = _g(16 + d)
    ref = (torch.randn(B, Nq, d, device=DEV, generator=g) * 2).to(dtype)
    ref[0, 0, :d] = torch.tensor([20.0, -20.0, 0.0, 8.0][:d])
    vr32 = 0.5 + 0.5 * torch.rand(B, L, 2, device=DEV, generator=g)
    vr = vr32.to(dtype)
    if with32:
        vr._codetr_f32 = vr32
    assert hip_ops.MSDA_FP32_REF and hip_ops.query_sine_embed_supported(ref, vr, 128)
    ref_in, emb = hip_ops.query_sine_embed(ref, vr, 128)
    u = U[dtype]
    tile = lambda v: torch.cat((v, v), -1) if d == 4 else v   # noqa: E731
    exact = torch.sigmoid(ref.double())[:, :, None] * tile(vr.double())[:, None]
    assert ref_in.shape == exact.shape and ref_in.dtype == dtype
    _within(ref_in, exact, 2 * u + u * u + 2.0 ** -19, 2 * TINY[dtype])
    ref32 = getattr(ref_in, "_codetr_ref32", None)
    if with32:
        assert ref32 is not None and ref32.dtype == torch.float32
        _within(ref32, torch.sigmoid(ref.double())[:, :, None] * tile(vr32.double())[:, None], 2.0 ** -21, 1e-38)
        coord = ref32[:, :, 0, :]
    else:
        assert ref32 is None
        coord = ref_in[:, :, 0, :].float()
    emb0 = DinoTransformerDecoder.gen_sineembed_for_position(coord, 128)
    assert emb.shape == (B, Nq, d * 128) and emb.dtype == dtype
    assert float((emb.float() - emb0).abs().max()) <= u + 1e-3
