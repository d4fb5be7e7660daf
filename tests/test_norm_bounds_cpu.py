"""The LayerNorm / GroupNorm bounds and the structured cases, proved on the CPU before a kernel is held to them
(tests/norm_bounds.py; the kernels run in tests/test_layernorm_gpu.py and tests/test_groupnorm_gpu.py).

(a) the emulation of each kernel's rounding points stays inside the bound on every input family the GPU modules run, at the
    same shapes and values;
(b) the fp32 part of the bound stays below u (|gamma| max(|xhat|, 1) + |beta|) / 4 on every family but the offset ones: the bound
    is the store rounding and cannot be inflated through the fp32 terms unnoticed.  On the offset families it is printed: there
    it is the conditioning of the problem (an fp32 mean of values near 100 is good to 1e-5, which is a fifth of sigma = 0.05);
(c) every mutant of the emulation leaves the bound in the family CATCH_* names, for fp16 and for bf16;
plus: no random case that existed before is held to less than its old rtol / atol, the structured cases' closed forms are what
the float64 reference gives, and the bf16 offset inputs still have a variance.

Run with -s to see the largest err / bound per family, the fp32 shares and the margin of every mutant."""
import math

import pytest
import torch

import norm_bounds as nb

F16, BF16 = torch.float16, torch.bfloat16
DT = {F16: "f16", BF16: "bf16"}
EPS = 1e-5

CATCH_LN = {"one_pass_variance": "offset", "unbiased_variance": "random", "eps_outside_sqrt": "two_valued",
            "stats_skip_last_chunk": "last_chunk", "stats_over_32_lanes_when_64": "random", "affine_chunk_shifted": "random",
            "normalised_rounded_before_affine": "random"}
CATCH_MERGE = {"swap_ky_kx": "merge", "pad_clamps_instead_of_zero": "merge", "row_decode_uses_W_not_W2": "merge"}
CATCH_GN = {"fp32_sums_no_pivot": "offset", "last_slab_dropped": "random", "count_uses_full_slabs": "random",
            "stats_of_previous_image": "random", "group_spans_16_channels": "random", "eps_outside_sqrt": "two_valued",
            "dest_ignores_batch_stride": "random"}
SENTINEL, ROW_START, EXTRA_ROWS = 7.0, 5, 13
# families with |mean| >> sigma (a constant row is the limit: sigma = 0), where the fp32 share is the problem's conditioning
ILL_CONDITIONED = ("offset", "constant")


def _ln_families(dtype):
    """(family, name, (x, gamma, beta))"""
    for C in nb.LN_EDGE_C + nb.LN_MODEL_C:
        for rows in nb.LN_ROWS:
            yield "random", f"{rows}x{C}", nb.ln_random(rows, C, dtype)
    for rows, C in nb.LN_GRID_STRIDE:
        yield "random", f"{rows}x{C}", nb.ln_random(rows, C, dtype)
    for mean, sigma, dt in nb.LN_OFFSET:
        if dt == dtype:
            yield "offset", f"{mean:g}+-{sigma:g}", nb.ln_offset(mean, sigma, dtype)
    for C in (256, 192):
        yield "constant", f"C{C}", nb.ln_constant(C, dtype)
        yield "two_valued", f"C{C}", nb.ln_two_valued(C, dtype)
    for C in nb.LN_LAST_CHUNK_C:
        yield "last_chunk", f"C{C}", nb.ln_last_chunk(C, dtype)


def _gn_families(dtype):
    """(family, name, (x, gamma, beta), groups)"""
    for groups in nb.GN_GROUPS:
        for HW in nb.GN_HW:
            yield "random", f"G{groups} HW{HW}", nb.gn_random(groups, HW, dtype), groups
    for mean, sigma in nb.GN_OFFSET[dtype]:
        yield "offset", f"{mean:g}+-{sigma:g}", nb.gn_offset(mean, sigma, dtype), 32
    yield "outlier", "token 0 at 50 sigma", nb.gn_outlier(dtype), 32
    yield "constant", "129 tokens", nb.gn_constant(dtype), 32
    yield "two_valued", "129 tokens", nb.gn_two_valued(dtype), 32


@pytest.fixture(scope="module")
def ln_cases():
    out = {}
    for dt in (F16, BF16):
        out[dt] = []
        for fam, name, x in _ln_families(dt):
            ex = nb.exact_layernorm(*x, EPS)
            out[dt].append((fam, name, x, ex, nb.bound_layernorm(ex)))
    return out


@pytest.fixture(scope="module")
def merge_cases():
    out = {}
    for dt in (F16, BF16):
        out[dt] = []
        for shape in nb.MERGE_SHAPES:
            x = nb.merge_input(*shape, dt)
            ex = nb.exact_patch_merge_layernorm(*x, EPS)
            out[dt].append(("merge", "x".join(map(str, shape)), x, ex, nb.bound_layernorm(ex)))
    return out


@pytest.fixture(scope="module")
def gn_cases():
    out = {}
    for dt in (F16, BF16):
        out[dt] = []
        for fam, name, x, groups in _gn_families(dt):
            ex = nb.exact_groupnorm_tokens(*x, groups, EPS)
            out[dt].append((fam, name, x, groups, ex, nb.bound_groupnorm(ex)))
    return out


def _gn_dest(x):
    B, HW, C = x.shape
    return torch.full((B, HW + EXTRA_ROWS, C), SENTINEL, dtype=x.dtype)


def _gn_ratio(x, groups, ex, b, mutant=None):
    dest = nb.emulate_groupnorm_tokens(*x, groups, EPS, mutant=mutant, dest=_gn_dest(x[0]), row_start=ROW_START)
    return nb.dest_ratio(dest, ROW_START, x[0].shape[1], SENTINEL, ex, b.total.view(ex.out.shape))


def _report(what, rows):
    """rows: (dtype, family, name, err/bound, fp32 share) -> prints the per-family maxima, asserts (a) and (b)"""
    worst, share = {}, {}
    for dt, fam, name, r, c in rows:
        key = f"{fam} {DT[dt]}"
        worst[key], share[key] = max(worst.get(key, 0.0), r), max(share.get(key, 0.0), c)
        assert r < 1, (what, fam, name, dt, r)
        if fam not in ILL_CONDITIONED:
            assert c < 1, (what, fam, name, dt, c)
    for key in worst:
        print(f"{what} {key}: largest emulated err/bound {worst[key]:.3f}, fp32 part / (u (|g| max(|xhat|, 1) + |b|) / 4) {share[key]:.3g}")


# ------------------------------------------------------------------------------------------------------- (a), (b)
def test_layernorm_emulation_inside_bound_on_every_family(ln_cases):
    rows = []
    for dt in (F16, BF16):
        for fam, name, x, ex, b in ln_cases[dt]:
            rows.append((dt, fam, name, nb.ratio(nb.emulate_layernorm(*x, EPS), ex.out, b.total), nb.fp32_share(ex, b)))
    _report("layernorm", rows)


def test_patch_merge_emulation_inside_bound(merge_cases):
    rows = []
    for dt in (F16, BF16):
        for fam, name, x, ex, b in merge_cases[dt]:
            rows.append((dt, fam, name, nb.ratio(nb.emulate_patch_merge_layernorm(*x, EPS), ex.out, b.total), nb.fp32_share(ex, b)))
    _report("patch merge", rows)


def test_groupnorm_emulation_inside_bound_on_every_family(gn_cases):
    rows = []
    for dt in (F16, BF16):
        for fam, name, x, groups, ex, b in gn_cases[dt]:
            rows.append((dt, fam, name, _gn_ratio(x, groups, ex, b), nb.fp32_share(ex, b)))
    _report("groupnorm", rows)


# ------------------------------------------------------------------------------------------------------- no weaker than before
def test_layernorm_bound_is_nowhere_above_the_tolerance_it_replaces():
    for dt in (F16, BF16):
        for rows, C in nb.LN_LEGACY:
            x = nb.ln_random(rows, C, dt)
            ex = nb.exact_layernorm(*x, EPS)
            b = nb.bound_layernorm(ex)
            frac = (b.total / nb.ln_legacy_tol(ex.out, dt)).max().item()
            print(f"layernorm {DT[dt]} {rows}x{C}: bound / old tolerance <= {frac:.3f}")
            assert frac <= 1, (rows, C, dt)
            if rows <= 1000:
                assert nb.ratio(nb.emulate_layernorm(*x, EPS), ex.out, b.total) < 1, (rows, C, dt)
    for mean, sigma, dt in nb.LN_OFFSET[:1]:                           # the offset test keeps rtol = atol = 2e-3 beside the bound
        ex = nb.exact_layernorm(*nb.ln_offset(mean, sigma, dt), EPS)
        print("layernorm offset: bound / (2e-3 |ref| + 2e-3) <=", (nb.bound_layernorm(ex).total / (2e-3 * ex.out.abs() + 2e-3)).max().item())
    x = nb.merge_input(*nb.MERGE_LEGACY_BF16, BF16)
    ex = nb.exact_patch_merge_layernorm(*x, EPS)
    assert (nb.bound_layernorm(ex).total <= 1e-2 * ex.out.abs() + 2e-2).all()


def test_groupnorm_bound_is_nowhere_above_the_tolerance_it_replaces():
    for B, HW in nb.GN_LEGACY_F16:
        x = nb.gn_legacy(B, HW, F16)
        ex = nb.exact_groupnorm_tokens(*x, 32, EPS)
        b = nb.bound_groupnorm(ex)
        frac = (b.total / (2.0 ** -10 * ex.out.abs() + 2e-3)).max().item()
        print(f"groupnorm f16 B{B} HW{HW}: bound / old tolerance <= {frac:.3f}")
        assert frac <= 1, (B, HW)
        if HW <= 10000:
            assert nb.ratio(nb.emulate_groupnorm_tokens(*x, 32, EPS), ex.out, b.total) < 1, (B, HW)
    x = nb.gn_legacy(*nb.GN_LEGACY_BF16, BF16)
    ex = nb.exact_groupnorm_tokens(*x, 32, EPS)
    b = nb.bound_groupnorm(ex)
    assert (b.total <= 1e-2 * ex.out.abs() + 2e-2).all()
    assert nb.ratio(nb.emulate_groupnorm_tokens(*x, 32, EPS), ex.out, b.total) < 1


# ------------------------------------------------------------------------------------------------------- (c)
def _caught(cases, run):
    """{family: ["name (margin x)"]} of the cases whose err / bound exceeds 1"""
    caught = {}
    for case in cases:
        r = run(case)
        if r > 1:
            caught.setdefault(case[0], []).append(f"{case[1]} ({r:.3g}x)")
    return caught


@pytest.mark.parametrize("mutant", nb.LN_MUTANTS)
def test_layernorm_mutant_is_caught(mutant, ln_cases):
    for dt in (F16, BF16):
        caught = _caught(ln_cases[dt], lambda c: nb.ratio(nb.emulate_layernorm(*c[2], EPS, mutant=mutant), c[3].out, c[4].total))
        print(f"layernorm {mutant} {DT[dt]}: caught by {caught}")
        assert CATCH_LN[mutant] in caught, (mutant, dt, caught)


@pytest.mark.parametrize("mutant", nb.MERGE_MUTANTS)
def test_patch_merge_mutant_is_caught(mutant, merge_cases):
    for dt in (F16, BF16):
        caught = _caught(merge_cases[dt],
                         lambda c: nb.ratio(nb.emulate_patch_merge_layernorm(*c[2], EPS, mutant=mutant), c[3].out, c[4].total))
        print(f"patch merge {mutant} {DT[dt]}: caught by {caught}")
        assert CATCH_MERGE[mutant] in caught, (mutant, dt, caught)


@pytest.mark.parametrize("mutant", nb.GN_MUTANTS)
def test_groupnorm_mutant_is_caught(mutant, gn_cases):
    for dt in (F16, BF16):
        caught = _caught(gn_cases[dt], lambda c: _gn_ratio(c[2], c[3], c[4], c[5], mutant=mutant))
        print(f"groupnorm {mutant} {DT[dt]}: caught by {caught}")
        assert CATCH_GN[mutant] in caught, (mutant, dt, caught)


def test_sums_without_a_pivot_are_caught_by_both_named_offset_families(gn_cases):
    """fp32 partials of x and x^2 alone (the kernel before it checked them) must leave the bound at 100 +- 0.25 and at 100 +- 0.05"""
    for dt in (F16, BF16):
        must = {f"{m:g}+-{s:g}" for m, s in nb.GN_OFFSET_MUST_CATCH[dt]}
        for fam, name, x, groups, ex, b in gn_cases[dt]:
            if fam == "offset":
                r = _gn_ratio(x, groups, ex, b, mutant="fp32_sums_no_pivot")
                mine = nb.bound_groupnorm(ex, resum=False).total
                print(f"groupnorm fp32 partials alone {DT[dt]} {name}: err/bound {r:.3g}; summed again: {(nb.gn_lost(ex) > 1).sum().item()}"
                      f" of {ex.mu.numel()} groups; the partials' own contract allows {(mine / b.total).max().item():.3g} x this bound")
                if name in must:
                    assert r > 1, (name, dt, r)
                    assert (nb.gn_lost(ex) > 1.001).all()
                    must.discard(name)
        assert not must, must


def test_both_branches_of_the_finalize_kernel_are_exercised(gn_cases):
    """the random family keeps the fp32 partials in many groups and flags many; the C = 256 inputs that existed before keep them
    everywhere, each in its own type (what they compute does not change)"""
    for dt in (F16, BF16):
        kept = again = 0
        for fam, name, x, groups, ex, b in gn_cases[dt]:
            z = nb.gn_lost(ex)
            if fam == "random":
                kept, again = kept + (z < 0.999).sum().item(), again + (z > 1.001).sum().item()
        print(f"groupnorm random {DT[dt]}: {kept} groups keep the fp32 partials, {again} are summed again")
        assert kept > 100 and again > 100
    for (B, HW), dt in [(c, F16) for c in nb.GN_LEGACY_F16[:4]] + [(nb.GN_LEGACY_BF16, BF16)]:
        ex = nb.exact_groupnorm_tokens(*nb.gn_legacy(B, HW, dt), 32, EPS)
        assert (nb.gn_lost(ex) < 0.999).all(), (B, HW, dt)


def test_non_finite_output_counts_as_wrong():
    x = nb.ln_random(7, 192, F16)
    ex = nb.exact_layernorm(*x, EPS)
    assert nb.ratio(torch.full_like(ex.out, math.nan), ex.out, nb.bound_layernorm(ex).total) == math.inf
    bad = ex.out.clone()
    bad[3, 5] = math.inf
    assert nb.ratio(bad, ex.out, nb.bound_layernorm(ex).total) == math.inf
    x = nb.gn_random(2, 127, BF16)
    exg = nb.exact_groupnorm_tokens(*x, 2, EPS)
    dest = _gn_dest(x[0])
    dest[:, ROW_START:ROW_START + 127] = math.nan
    assert nb.dest_ratio(dest, ROW_START, 127, SENTINEL, exg, nb.bound_groupnorm(exg).total) == math.inf
    dest = nb.emulate_groupnorm_tokens(*x, 2, EPS, dest=_gn_dest(x[0]), row_start=ROW_START)
    dest[1, ROW_START - 1, 3] = 0                                      # a neighbour overwritten
    assert nb.dest_ratio(dest, ROW_START, 127, SENTINEL, exg, nb.bound_groupnorm(exg).total) == math.inf


# ------------------------------------------------------------------------------------------------------- the constructions
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_structured_expectations_in_closed_form(dtype):
    for C in (256, 192):
        x, gamma, beta = nb.ln_constant(C, dtype)
        assert (x.double() == torch.tensor(nb.LN_CONSTANTS, dtype=torch.float64).view(-1, 1)).all()    # exact in the type
        ex = nb.exact_layernorm(x, gamma, beta, EPS)
        assert (ex.out - beta.double()).abs().max() < 1e-12
        if C == 256:
            assert torch.equal(nb.emulate_layernorm(x, gamma, beta, EPS), beta.expand_as(x))
        x, gamma, beta = nb.ln_two_valued(C, dtype)
        m = torch.tensor([m for m, _ in nb.LN_TWO_VALUED], dtype=torch.float64)
        d = torch.tensor([d for _, d in nb.LN_TWO_VALUED], dtype=torch.float64)
        assert ((x.double() - m[:, None]).abs() == d[:, None]).all()                                    # m +- d survived the type
        ex = nb.exact_layernorm(x, gamma, beta, EPS)
        assert (ex.out - nb.ln_two_valued_expected(C, gamma, EPS)).abs().max() < 1e-12
        assert (gamma.double().abs().log2() % 1 == 0).all()
    for C in nb.LN_LAST_CHUNK_C:
        x, gamma, beta = nb.ln_last_chunk(C, dtype)
        assert (x[:, :-8] == 0).all() and (x[:, -8:] != 0).all()
        ex = nb.exact_layernorm(x, gamma, beta, EPS)
        assert (ex.out - nb.ln_last_chunk_expected(x, gamma, beta, EPS)).abs().max() < 1e-12
    x, gamma, beta = nb.gn_constant(dtype)
    assert (nb.exact_groupnorm_tokens(x, gamma, beta, 32, EPS).out - beta.double().view(32, 8)).abs().max() < 1e-12
    assert torch.equal(nb.emulate_groupnorm_tokens(x, gamma, beta, 32, EPS), beta.expand_as(x))
    assert x.double().view(3, 129, 32, 8).std((1, 3)).max() == 0 and x.unique().numel() > 32
    x, gamma, beta = nb.gn_two_valued(dtype)
    ex = nb.exact_groupnorm_tokens(x, gamma, beta, 32, EPS)
    assert (ex.out - nb.gn_two_valued_expected(gamma, beta, EPS)).abs().max() < 1e-12
    assert (ex.var.flatten(1) == (2.0 ** (2 * (torch.arange(3.0) - 8)))[:, None]).all()


def test_patch_merge_gather_indices_equal_the_padded_views():
    for shape in nb.MERGE_SHAPES + [nb.MERGE_LEGACY_BF16]:
        x, _, _ = nb.merge_input(*shape, F16)
        assert torch.equal(nb.merge_gather(x), nb.exact_patch_merge(x))
    x, _, _ = nb.merge_input(2, 7, 9, 192, F16)
    for mutant in nb.MERGE_MUTANTS:
        assert not torch.equal(nb.merge_gather(x, mutant), nb.exact_patch_merge(x))


def test_offset_inputs_keep_a_variance_in_bf16():
    """at least three distinct values survive the type in every (image, group) of every offset family"""
    for dt in (F16, BF16):
        for mean, sigma in nb.GN_OFFSET[dt]:
            x, _, _ = nb.gn_offset(mean, sigma, dt)
            xg = x.float().view(nb.GN_B, 300, 32, 8).permute(0, 2, 1, 3).reshape(nb.GN_B * 32, -1)
            fewest = min(row.unique().numel() for row in xg)
            rho = (x.double().mean() ** 2 / x.double().view(nb.GN_B, 300, 32, 8).var((1, 3)).mean()).item()
            print(f"groupnorm offset {DT[dt]} {mean:g}+-{sigma:g}: at least {fewest} distinct values per group, mean^2 / var = {rho:.3g}")
            assert fewest >= 3, (mean, sigma, dt)


def test_dispatch_edges_are_the_launchers():
    """ln_config restates `launch` of csrc/layernorm.hip: one C on either side of every edge"""
    want = {8: (32, 1), 256: (32, 1), 264: (64, 1), 512: (64, 1), 520: (64, 2), 1024: (64, 2), 1032: (64, 3), 1536: (64, 3),
            1544: (64, 4), 2048: (64, 4), 2056: (64, 6), 3072: (64, 6), 3080: (64, 8), 4096: (64, 8)}
    for C, cfg in want.items():
        assert nb.ln_config(C) == cfg
        assert cfg[0] * cfg[1] * 8 >= C
    assert [nb.gn_depth(g) for g in nb.GN_GROUPS] == [8 * 1 + 256, 8 * 1 + 128, 8 * 16 + 8, 8 * 32 + 4, 8 * 128 + 1]
