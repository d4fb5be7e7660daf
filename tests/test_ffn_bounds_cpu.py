"""tests/ffn_bounds.py on the CPU: the fp32 emulation of the fused FFN / Swin MLP kernels stays inside the derived bound on
every case the GPU tests run, the exact-integer cases are exact, the launch plans put every case on the kernel form its name
claims, and every mutant is caught by a named case -- by the bound, or by the share of elements that differ from the exact
value against 4 x the emulation's share (with the cap at least 10 x below the mutant's share).  The row counts are those of a
part with CUS compute units; the plan claims are also checked at the MI355X's 256."""
import pytest
import torch

import ffn_bounds as fb

CUS = 6
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
ALL = [("ffn", n) for n in fb.FFN_CASE_NAMES] + [("swin", n) for n in fb.SWIN_CASE_NAMES]

# mutant -> the cases that must catch it, in both types
FFN_CATCHES = {
    "hidden_truncated": ("coherent_h64", "coherent_h512", "tails_h64_plain", "tails_h2048_plain"),
    "hidden_kept_fp32": ("tails_h64_plain", "tails_h2048_plain"),
    "y_not_rounded_before_residual": ("tails_h64_plain", "tails_h2048_plain"),
    "w2_unpacked": ("routing0_tails_plain_pos", "routing1_tails_plain_pos"),
    "oproj_w1_unpermuted": ("routing0_tails_oproj_plain", "routing1_tails_oproj_plain"),
    "stale_ring_stage": ("multi_h128_plain", "multi_h192_plain", "multi_h128_oproj", "multi_h192_oproj"),
    "last_chunk_dropped": ("multi_h64_plain", "multi_h192_plain"),
    "ln_in_reads_ln_params": ("distinct_small", "distinct_ragged"),
    "one_pass_variance": ("distinct_small",),
    "identity_is_raw_x_under_ln_in": ("tails_h64_full",),
    "pos_added_before_ln": ("tails_h64_full",),
    "second_launch_ignores_row_offset": ("split_full", "split_oproj", "exact_split_plain_pos", "exact_split_oproj_plain"),
}
SWIN_CATCHES = {
    "hidden_truncated": ("coherent_c192", "coherent_c384", "tails_c192"),
    "hidden_kept_fp32": ("tails_c192", "tails_c384"),
    "y_not_rounded_before_residual": ("tails_c192", "tails_c384"),
    "w2_unpacked": ("tails_c192", "tails_c384"),
    "stale_ring_stage": ("walk_c192", "walk_c384"),
    "last_chunk_dropped": ("tails_c192", "tails_c384"),
    "one_pass_variance": ("offset_c192", "offset_c384"),
    "swin_residual_is_normed_x": ("tails_c192", "walk_c384"),
}
# the hidden = 64 and the coherent cases catch a truncating pack by the bound alone
TRUNCATION_BY_BOUND = ("coherent_h64", "coherent_h512", "tails_h64_plain")


def _cases(kind, cus=CUS):
    return fb.ffn_cases(cus) if kind == "ffn" else fb.swin_cases(cus)


@DTYPES
@pytest.mark.parametrize("kind,name", ALL)
def test_emulation_is_inside_the_bound(kind, name, dtype):
    case = _cases(kind)[name]
    res = fb.measure(case, dtype, lambda inp: fb.emulate(inp, None, CUS), "cpu", CUS)
    print(f"{kind} {name} {dtype}: err/bound {res.ratio:.3f} share {res.share:.5f}")
    assert res.ratio <= 1.0


@DTYPES
@pytest.mark.parametrize("name", [n for n in fb.FFN_CASE_NAMES if n.startswith(("exact", "routing"))])
def test_integer_cases_are_exact(name, dtype):
    """every intermediate and output of the float64 reference is an integer the storage type holds.  The bound is 0 nearly
    everywhere but not at and next to the zeros (the storage types have no coarse step there to absorb the accumulation
    radius), so the GPU tests ask these cases for equal bits; it is far below the distance to another integer"""
    case = fb.ffn_cases(CUS)[name]
    for M in case.Ms:
        ex = fb.exact_ffn(fb.build(case, M, dtype))
        for stage, v in ex.stages:
            assert bool((v == v.round()).all()) and float(v.abs().max()) <= fb.INT_LIMIT[dtype], (stage, float(v.abs().max()))
        b = fb.bound(ex)
        for v, r in ((ex.out, b.out), (ex.out2, b.out2)):
            assert float((r == 0).double().mean()) > 0.5 and float(r.max()) < 0.01
    if name.startswith("routing"):
        R, Cm = fb.ROUTING[dtype][int(case.build[-1])]
        assert fb.build(case, 16, dtype)["x"].double().unique().numel() == R * Cm      # one integer per (row mod R, column mod Cm)


@DTYPES
@pytest.mark.parametrize("kind,table", [("ffn", FFN_CATCHES), ("swin", SWIN_CATCHES)])
def test_every_mutant_is_caught(kind, table, dtype):
    assert set(table) == set(fb.FFN_MUTANTS if kind == "ffn" else fb.SWIN_MUTANTS)
    for mutant, names in table.items():
        for name in names:
            res = fb.measure(_cases(kind)[name], dtype, lambda inp: fb.emulate(inp, mutant, CUS), "cpu", CUS)
            print(f"{kind} {mutant} on {name} {dtype}: err/bound {res.ratio:.3g} share {res.share:.4f} cap {fb.share_cap(res):.5f}")
            assert not fb.holds(res), (mutant, name)
            # the biased rounding that the share criterion exists for: the cap is nowhere near its share.  (A hidden activation
            # kept in fp32 and a y that is not rounded flip 15 - 29 % at hidden >= 768, 4 - 9 x the fp16 cap there.)
            if mutant == "hidden_truncated":
                assert 10 * fb.share_cap(res) <= res.share, (mutant, name, res)
            if mutant == "hidden_truncated" and name in TRUNCATION_BY_BOUND:
                assert res.ratio > 1.0, (name, res)


@pytest.mark.parametrize("cus", [256, CUS, 304])
def test_plans_put_every_case_on_the_form_its_name_claims(cus):
    for case in fb.ffn_cases(cus).values():
        for M in case.Ms:
            plan = fb.ffn_plan(M, case.hidden, cus)
            assert tuple(l.form for l in plan.launches) == case.forms and plan.walk == case.walk, (case.name, M, plan)
            assert plan.nchunks == case.hidden // 64
            assert sum(l.rows for l in plan.launches) == M and plan.launches[0].row0 == 0
            for l in plan.launches:
                assert l.form == 128 or l.walk == 1          # the 64-row form never walks a second tile
    for case in fb.swin_cases(cus).values():
        for M in case.Ms:
            plan = fb.swin_plan(M, case.form, cus)
            assert plan.walk == case.walk and plan.nchunks % 2 == 0, (case.name, M, plan)
    # what the issue's arithmetic says of the row counts themselves
    assert fb.ffn_plan(64 * cus, 2048, cus).launches[0].form == 64            # up to 64 x CUs rows: the 64-row form alone
    assert fb.ffn_plan(128 * cus, 2048, cus).walk == 1 and fb.ffn_plan(128 * cus + 128 * (cus // 2 + 1), 2048, cus).walk == 2
    ragged = fb.ffn_plan(fb.ragged_M(cus), 2048, cus).launches[0]
    assert 64 < ragged.rows - 128 * (ragged.ntiles - 1) < 96                  # the last tile ends inside wave 2
    split = fb.ffn_plan(fb.split_M(cus), 2048, cus).launches
    assert (split[1].row0, split[1].rows, split[1].ntiles) == (128 * cus, 197, 4)
    assert [c % 2 for c in (1, 2, 3)] == [fb.ffn_plan(fb.multi_M(cus), h, cus).nchunks % 2 for h in (64, 128, 192)]


def test_index_restatements_are_permutations():
    assert sorted(fb.pack_w2_index(192).tolist()) == list(range(192))
    assert sorted(fb.oproj_w1_index().tolist()) == list(range(256))
    assert fb.pack_w2_index(64)[:16].tolist() == [0, 1, 2, 3, 16, 17, 18, 19, 4, 5, 6, 7, 20, 21, 22, 23]
