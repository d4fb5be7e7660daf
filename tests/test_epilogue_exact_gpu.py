"""Every copy of the GEMM epilogue against its contract, bit for bit, on inputs that determine the output exactly
(tests/epilogue_exact.py; the construction itself is checked by tests/test_epilogue_exact_cpu.py):

    y = E(E(act(acc + bias)) + r),   act 3: E(relu(E(acc + bias) + r)),   row state 1 -> 0 (+ r), 2 -> E(act(bias)) (+ r)

None, ReLU, relu_res and the row states are compared as int16 (a NaN as any NaN); GELU by the interval of
`epilogue_exact.gelu_accept` (a = 4.8e-7 |z| around float64 0.5 z erfc(-z / sqrt 2)).  The x rows are one-hot (set A:
every 16-bit value as one product; set B: quarter ulps from the bias; set B2: quarter ulps from a second product, bias in
{0, ulp / 4}, residual in {none, 3/8 ulp, -0.75 v}), so no tolerance is involved.  B2 relies on the 16x16x32 matrix
instruction returning a sum exactly when every partial sum is fp32-representable.

Each copy is reached at the smallest shape its kernel accepts, asked from the library (codetr_linear_variant,
codetr_linear_splitk_plan, codetr_linear_{sk,pp}_supported), and the kernel that served is asserted:
the 128-tile kernel (vector and ragged-N stores, head-major, act 3, row states), the 256-tile kernel (act 3, row states),
the X-stationary kernel (row-major, head-major, bf16 operands -> fp16, row states), the split-K second pass (row states),
the persistent kernel (resident, one workgroup per tile, stream-K split), the ping-pong kernel, and the fused FFN.

Measured on an MI355X: zero differing bits on every None / ReLU / relu_res / row-state case of every route, every GELU
output inside its interval.  The GELU error itself is only visible through a 16-bit output: the part of |y - gelu(z)| that
half an ulp of the result cannot explain (`gelu_accept`'s second value, a lower bound on the error of the fp32 formula as
run) peaks at 7.134e-08 |z| for fp16 outputs and 2.237e-08 |z| for bf16 outputs, the same on all nine routes -- below the
emulation's 2.4e-7 |z|, so nothing to explain.  Findings of the first run: the fused FFN's packed ReLU dropped a NaN hidden
unit (fixed: relu_bits16 in csrc/device_prims.h); gelu_erf and gelu_erf2 do not always STORE the same fp16 bits (4 of
184 326 set-A inputs; see test_gelu_erf_and_gelu_erf2_agree).  Sets B and B2 pass on every route: the matrix instruction
returned every exactly representable sum exactly.
"""
import functools

import pytest
import torch

import epilogue_exact as ee

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]

# route -> K, column alignment, extra columns (ragged N), fewest rows, most columns per launch
ROUTES = {
    "tile128": dict(K=64, align=8),
    "tile128_ragged": dict(K=64, align=8, extra=1),
    "tile256": dict(K=256, align=256),
    "xs": dict(K=192, align=8, min_m=128 * 256 + 40, max_n=1536),
    "splitk": dict(K=2112, align=8, max_n=128),
    "sk": dict(K=128, align=8, flags=0),
    "sk_tile_per_wg": dict(K=128, align=8, flags=0x20),
    "sk_stream_k": dict(K=128, align=8, flags=0x40),
    "pp": dict(K=128, align=8),
}


@functools.lru_cache(maxsize=None)
def _case(kind, T, K):
    if kind == "A":
        return ee.set_a(T, K, DEV)
    if kind == "A_nobias":
        return ee.set_a(T, K, DEV, nonfinite_bias=False)
    if kind == "B":
        return ee.set_r(T, K, DEV, bias_js=(0, 1, 2, 3), x_js=(0,))
    return ee.set_r(T, K, DEV)


def _variant_rows(case_rows, N, K, want):
    """the first row count >= case_rows (in steps of 256) that codetr_linear_* serves with kernel `want`"""
    from codetr import _cabi

    M = case_rows
    while _cabi.linear_variant(M, N, K) != want:
        M += 256
        assert M < (1 << 20), f"no row count routes ({N}, {K}) to {want}"
    return M


def _launch(route, x, w, b, r, act, state):
    """one launch through the epilogue copy `route`; asserts which kernel served"""
    from codetr import _cabi

    M, K = x.shape
    N = w.shape[0]
    y = torch.full((M, N), float("nan"), dtype=x.dtype, device=DEV)
    before = dict(_cabi.CALLS)
    if route in ("tile128", "tile128_ragged", "tile256", "xs"):
        want = {"tile128_ragged": "tile128"}.get(route, route)
        assert _cabi.linear_variant(M, N, K, act, r is not None, 0) == want
        assert (N % 8 != 0) == (route == "tile128_ragged") and (route != "tile128_ragged" or N % 4 != 0)
        _cabi.linear(x, w, b, r, act, y, state)
        assert _cabi.CALLS["linear_" + want] == before["linear_" + want] + 1
    elif route == "splitk":
        splits, nbytes = _cabi.linear_splitk_plan(M, N, K)
        assert splits > 1
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _cabi.linear_splitk(x, w, b, r, act, y, splits, ws, state)
        assert _cabi.CALLS["linear_splitk"] == before["linear_splitk"] + 1
    elif route.startswith("sk"):
        assert state is None and _cabi.load().codetr_linear_sk_supported(M, N, K) == 1
        flags = ROUTES[route]["flags"]
        if flags & 0x40:
            ws = _cabi.linear_sk_workspace(torch.device(DEV))
            ws.zero_()
        _cabi.linear_sk(x, w, b, r, act, y, flags=flags)
        assert _cabi.CALLS["linear_sk"] == before["linear_sk"] + 1
        if flags & 0x40:
            # the split really engaged: partial sums went through the slabs (gemm_sk.hip: with fewer tiles than workgroups
            # and K = 128 every tile is cut into its two k-tiles), and the ticket counters are back at zero
            G = ws.numel() // (2 * 8 * 8192 * 4 + 8 * 4)
            slabs = G * 2 * 8 * 8192 * 4
            assert bool(ws[:slabs].any()) and not bool(ws[slabs:].any())
    else:
        assert route == "pp" and state is None and _cabi.load().codetr_linear_pp_supported(M, N, K) == 1
        _cabi.linear_pp(x, w, b, r, act, y)
        assert _cabi.CALLS["linear_pp"] == before["linear_pp"] + 1
    return y


GELU_EXCESS = {}


def _check(route, T, kind, act, bias=True, rmode=None, states=False):
    """the case set `kind` through `route`: zero differing bits (GELU: every output inside its interval)"""
    cfg = ROUTES[route]
    K = cfg["K"]
    full = _case(kind, T, K)
    n0 = full["w"].shape[0]
    step = cfg.get("max_n", n0)
    for lo in range(0, n0, step):
        case = ee.take_columns(full, lo, min(lo + step, n0))
        n = case["w"].shape[0]
        N = (n + cfg["align"] - 1) // cfg["align"] * cfg["align"] + cfg.get("extra", 0)
        case = ee.pad_columns(case, N)
        M = max(case["k1"].numel(), cfg.get("min_m", 0))
        if route == "tile256":
            M = _variant_rows(M, N, K, "tile256")
        x, w = ee.make_x(case, M), case["w"]
        b = case["b"] if bias else None
        r = ee.residual(case, M, rmode) if rmode else None
        state = (torch.arange(M, device=DEV) % 3).to(torch.uint8) if states else None
        y = _launch(route, x, w, b, r, act, state)
        acc = ee.accumulators(case, M)
        if act == "gelu":
            z = ee.pre_activation(acc, b, state)
            ok, excess = ee.gelu_accept(y, z, T, r)
            if state is not None:    # rows of state 1: the linear output is zero whatever the activation
                zero = ee.canonical_bits(y) == ee.canonical_bits(ee.expected(torch.zeros_like(acc), None, r, None, T))
                ok = torch.where((state == 1)[:, None], zero, ok)
            key = (route, str(T))
            GELU_EXCESS[key] = max(GELU_EXCESS.get(key, 0.0), excess)
            print(f"gelu {route} {T}: max unexplained |err| / |z| = {excess:.3e}")
            assert bool(ok.all()), (route, T, int((~ok).sum()), z[~ok][:8], y[~ok][:8])
        else:
            want = ee.expected(acc, b, r, act, T, state)
            bad = ee.canonical_bits(y) != ee.canonical_bits(want)
            print(f"{route} {T} {kind} act={act} bias={bias} res={rmode} states={states}: {int(bad.sum())} of {bad.numel()} differ")
            assert not bad.any(), (route, T, kind, act, int(bad.sum()), acc[bad][:8], y[bad][:8], want[bad][:8])


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_values(route, T):
    """set A: every 16-bit value (and +-inf, NaN through the bias) as the pre-activation"""
    _check(route, T, "A_nobias", None, bias=False)
    _check(route, T, "A", None)
    _check(route, T, "A", "relu")
    _check(route, T, "A", "gelu")


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_rounding(route, T):
    """sets B and B2: ties, quarter ulps either side, both signs, every binade; the residual added to the ROUNDED result"""
    _check(route, T, "B", None)
    _check(route, T, "B2", None, bias=False)
    _check(route, T, "B2", None, rmode="mix")
    _check(route, T, "B2", "relu", rmode="mix")


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("route", ["tile128", "tile128_ragged"])
def test_relu_after_the_residual_and_row_states_tile128(route, T):
    _check(route, T, "B2", "relu_res", rmode="mix")
    _check(route, T, "A", "relu_res")                      # no residual: act 3 is act 1
    for act in (None, "relu", "gelu"):
        _check(route, T, "A", act, states=True)
    _check(route, T, "B2", None, rmode="mix", states=True)
    _check(route, T, "B2", "relu_res", rmode="mix", states=True)


@pytest.mark.parametrize("T", DTYPES)
def test_relu_after_the_residual_and_row_states_xs(T):
    _check("xs", T, "B2", "relu_res", rmode="mix")
    for act in (None, "relu", "gelu"):
        _check("xs", T, "A", act, states=True)
    _check("xs", T, "B2", None, rmode="mix", states=True)


@pytest.mark.parametrize("T", DTYPES)
def test_relu_after_the_residual_and_row_states_tile256(T):
    _check("tile256", T, "B2", "relu_res", rmode="mix")
    _check("tile256", T, "A", "relu_res")                  # no residual: act 3 is act 1
    for act in (None, "relu", "gelu"):
        _check("tile256", T, "A", act, states=True)
    _check("tile256", T, "B2", None, rmode="mix", states=True)
    _check("tile256", T, "B2", "relu_res", rmode="mix", states=True)


@pytest.mark.parametrize("T", DTYPES)
def test_row_states_splitk(T):
    """the second pass takes None / relu / gelu (no act 3): row states under each, without and with a residual"""
    for act in (None, "relu", "gelu"):
        _check("splitk", T, "A", act, states=True)
        _check("splitk", T, "B2", act, rmode="mix", states=True)


@pytest.mark.parametrize("T", DTYPES)
def test_tile128_head_major(T):
    """the head-major destination of the 128-tile kernel (too few rows for the X-stationary one), with row states"""
    from codetr import _cabi, hip_ops

    K, hd, B, S = 64, 32, 2, 200
    case = _case("A", T, K)
    N = (case["w"].shape[0] + hd - 1) // hd * hd
    case = ee.pad_columns(case, N)
    M = B * S
    assert M < 128 * 256 and _cabi.linear_variant(M, N, K, None, False, hd) == "tile128"
    state = (torch.arange(M, device=DEV) % 3).to(torch.uint8)
    before = _cabi.CALLS["linear_tile128"]
    y = hip_ops.linear(ee.make_x(case, M).view(B, S, K), case["w"], case["b"], row_mask=state.view(B, S), head_major=hd)
    assert _cabi.CALLS["linear_tile128"] == before + 1 and y.shape == (B, N // hd, S, hd)
    want = ee.expected(ee.accumulators(case, M), case["b"], None, None, T, state)
    want = want.view(B, S, N // hd, hd).permute(0, 2, 1, 3)
    assert ee.differing(y, want.contiguous()) == 0


def _head_major_case(T, kind, p_out=None):
    K, N, hd, B = 256, 256, 32, 2
    case = ee.set_a(T, K, DEV) if kind == "A" else ee.set_r(T, K, DEV, bias_js=(0, 1, 2, 3), x_js=(0,), p_out=p_out)
    assert case["w"].shape[0] <= N
    case = ee.pad_columns(case, N)
    S = (128 * 256 + 80) // B
    M = B * S
    state = (torch.arange(M, device=DEV) % 3).to(torch.uint8)
    return case, ee.make_x(case, M).view(B, S, K), state, (B, S, N // hd, hd)


@pytest.mark.parametrize("T", DTYPES)
def test_xs_head_major(T):
    from codetr import _cabi, hip_ops

    # (set A: the rounding sets need more than this launch's 256 columns and run on this kernel's row-major form)
    case, x, state, (B, S, H, hd) = _head_major_case(T, "A")
    assert _cabi.linear_variant(B * S, H * hd, 256, None, False, hd) == "xs"
    before = _cabi.CALLS["linear_xs"]
    y = hip_ops.linear(x, case["w"], case["b"], row_mask=state.view(B, S), head_major=hd)
    assert _cabi.CALLS["linear_xs"] == before + 1 and y.shape == (B, H, S, hd)
    want = ee.expected(ee.accumulators(case, B * S), case["b"], None, None, T, state)
    want = want.view(B, S, H, hd).permute(0, 2, 1, 3)
    assert ee.differing(y, want.contiguous()) == 0


def test_value_projection_bf16_operands_fp16_result():
    """codetr_linear_bf16_f16out: ONE rounding of acc + bias to fp16 (set A of bf16; set B with fp16 quarter ulps)"""
    from codetr import _cabi, hip_ops

    for kind in ("A", "B"):
        case, x, state, (B, S, H, hd) = _head_major_case(torch.bfloat16, kind, p_out=10)
        before = _cabi.CALLS["linear_xs"]
        y = hip_ops.value_projection_f16(x, case["w"], case["b"], state.view(B, S), hd)
        assert y is not None and y.dtype == torch.float16 and _cabi.CALLS["linear_xs"] == before + 1
        want = ee.expected(ee.accumulators(case, B * S), case["b"], None, None, torch.float16, state)
        want = want.view(B, S, H, hd).permute(0, 2, 1, 3)
        assert ee.differing(y, want.contiguous()) == 0, kind


def _ffn_case(T):
    # set A without the products that leave the range: an inf hidden unit times a zero of w2 is a NaN in every output
    case = ee.set_a(T, 256, DEV, nonfinite_bias=False, scales=ee.row_scales_a(T)[:-1] if T == torch.float16 else [1.0])
    hidden = (case["w"].shape[0] + 63) // 64 * 64
    case = ee.pad_columns(case, hidden)
    M = case["k1"].numel()
    w2 = torch.zeros(256, hidden, dtype=T, device=DEV)
    unit = torch.arange(256, device=DEV)
    return case, M, hidden, w2, unit


@pytest.mark.parametrize("T", DTYPES)
def test_ffn_fused(T):
    """E(E(E(relu(x W1^T + b1)) W2^T + b2) + x): x one-hot, w1 enumerates set A, w2 one-hot onto hidden units (256 of them per
    launch), bit for bit"""
    from codetr import _cabi, hip_ops

    case, M, hidden, w2, unit = _ffn_case(T)
    x = ee.make_x(case, M)
    b1 = torch.zeros(hidden, dtype=T, device=DEV)
    b2 = torch.zeros(256, dtype=T, device=DEV)
    h = ee.expected(ee.accumulators(case, M), b1, None, "relu", T)          # [M, hidden]
    for first in range(0, hidden, 256):
        w2.zero_()
        sel = (first + unit) % hidden
        w2[unit, sel] = 1
        before = _cabi.CALLS["ffn_fused"]
        y = hip_ops.ffn_fused(x, case["w"], b1, w2.clone(), b2)
        assert _cabi.CALLS["ffn_fused"] == before + 1
        want = ee.expected(h[:, sel].float() + 0.0, b2, x, None, T)
        assert ee.differing(y, want) == 0, first


@pytest.mark.parametrize("T", DTYPES)
def test_ffn_fused_hidden_nan_propagates(T):
    """a NaN hidden unit (here from b1) is a NaN of relu, hence of every output of the row: relu is x < 0 ? 0 : x"""
    from codetr import hip_ops

    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(130, 256, device=DEV, generator=g).to(T)
    w1 = (torch.randn(64, 256, device=DEV, generator=g) / 16).to(T)
    w2 = (torch.randn(256, 64, device=DEV, generator=g) / 8).to(T)
    b2 = torch.zeros(256, dtype=T, device=DEV)
    for nan in (float("nan"), -float("nan")):
        b1 = torch.zeros(64, dtype=T, device=DEV)
        b1[5] = nan
        y = hip_ops.ffn_fused(x, w1, b1, w2, b2)
        assert bool(y.isnan().all()), int(y.isnan().sum())


@pytest.mark.parametrize("T", DTYPES)
def test_gelu_erf_and_gelu_erf2_agree(T):
    """the tile kernel (gelu_erf) and both persistent kernels (gelu_erf2) on set A.  Both persistent kernels give the same
    bits.  Against the tile kernel: identical in bf16; in fp16 the tile kernel's last fma and its conversion are one
    instruction (v_fma_mixlo_f16, one rounding) where the packed form rounds to fp32 first, so a double-rounding case may
    differ -- by one fp16 ulp at most, and both values lie inside the GELU interval (test_values)."""
    case = ee.pad_columns(_case("A", T, 128), (_case("A", T, 128)["w"].shape[0] + 7) // 8 * 8)
    M = case["k1"].numel()
    x = ee.make_x(case, M)
    ys = {route: _launch(route, x, case["w"], case["b"], None, "gelu", None) for route in ("tile128", "sk", "pp")}
    assert ee.differing(ys["pp"], ys["sk"]) == 0
    if T == torch.bfloat16:
        assert ee.differing(ys["sk"], ys["tile128"]) == 0
        return
    a, b = ee.canonical_bits(ys["sk"]).int(), ee.canonical_bits(ys["tile128"]).int()
    print("fp16 gelu_erf2 vs gelu_erf:", int((a != b).sum()), "of", a.numel(), "differ")
    assert int((a - b).abs().max()) <= 1        # (bit patterns of one sign are consecutive; +-0 never differ here)
    z = ee.pre_activation(ee.accumulators(case, M), case["b"])
    for y in ys.values():
        assert bool(ee.gelu_accept(y, z, T)[0].all())
