"""tests/decoder_layer_bounds.py on the CPU: the fp32 emulation of codetr_decoder_layer passes every case the GPU test runs, in
both types; the probe cases are what they claim (exact gathers, every point selected, every border position hit, integer stages,
all eight chunk rotations); every probe bound is finite for every element; every mutant of DEC_MUTANTS fails a named case; the
weight blobs unpack to the weights they were packed from; the (L, P) table is dims_ok's."""
import numpy as np
import pytest
import torch

import decoder_layer_bounds as db

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])

# mutant -> the cases that must catch it, in both types
CATCHES = {
    "corner_index_transposed": ("gather_exact_L5P4", "gather_exact_L2P8"),
    "level_start_ignored": ("gather_exact_L5P4", "gather_exact_L3P4"),
    "row_image_is_tile_image": ("gather_exact_L5P4", "gather_exact_L1P2"),
    "gate_inclusive": ("gather_exact_L5P4", "gather_exact_L4P4"),
    "border_corner_kept": ("gather_exact_L5P4", "gather_exact_L4P4"),
    "offset_xy_swapped": ("gather_exact_L5P4", "gather_exact_L5P2"),
    "offset_scale_without_half": ("gather_exact_L5P4", "gather_exact_L2P8"),
    "wh_taken_from_xy": ("gather_exact_L5P4", "gather_exact_L1P2"),
    "valid_ratio_of_level0_everywhere": ("gather_exact_L5P4", "gather_exact_L5P2"),
    "softmax_per_level": ("gather_exact_L5P4", "gather_exact_L4P4"),
    "logit_columns_point_major": ("gather_exact_L5P4", "gather_exact_L2P8"),
    "points_beyond_ten_dropped": ("gather_exact_L5P4", "gather_exact_L4P4", "gather_exact_L3P4", "gather_exact_L2P8"),
    "head_stride_wrong": ("gather_exact_L5P4", "gather_exact_L1P2"),
    "oproj_not_rounded_before_residual": ("oproj_exact",),
    "q2_without_qpos": ("gather_exact_L5P4", "random_L5P4_head"),
    "b1_chunk_not_rotated": ("ffn_exact",),
    "w2_chunk_not_rotated": ("ffn_exact",),
    "last_chunk_dropped": ("ffn_exact", "random_L5P4_tail"),
    "hidden_kept_fp32": ("ffn_rounding",),
    "pre_ln3_rounded": ("ffn_rounding",),
    "ffn_residual_is_x1": ("ffn_exact", "random_L5P4_head"),
    "one_pass_variance": ("ffn_rounding",),
    "final_norm_skipped": ("box_exact_tail", "random_L5P4_tail"),
    "ref_added_before_rounding": ("box_exact_head", "box_exact_tail"),
    "sine_xy_order": ("sine_exact",),
    "sine_uses_own_level_ratio": ("sine_exact",),
    "sine_of_unrefined_ref": ("random_L5P4_head", "random_L4P5_head"),
    "temperature_natural_log": ("sine_exact",),
    "k_without_qpos": ("random_L5P4_head", "random_L1P2_head"),
    "v_with_qpos": ("random_L5P4_head", "box_exact_head"),
}


@DTYPES
@pytest.mark.parametrize("name", db.CASE_NAMES)
def test_emulation_passes_every_case(name, dtype):
    fig = db.hold(name, dtype, db.emulate)
    print(f"{name} {dtype}: {fig}")


@DTYPES
def test_every_mutant_is_caught(dtype):
    assert set(CATCHES) == set(db.DEC_MUTANTS)
    table = []
    for mutant, names in CATCHES.items():
        for name in names:
            with pytest.raises(AssertionError):
                db.hold(name, dtype, lambda inp: db.emulate(inp, mutant))
            table.append(f"{mutant:36s} {name}")
    print(f"{dtype}: mutant -> case that catches it\n" + "\n".join(table))


@DTYPES
@pytest.mark.parametrize("L,P", db.LP_PROBES)
def test_gather_exact_is_what_it_claims(L, P, dtype):
    inp = db.gather_exact(dtype, L, P)
    ex = db.exact(inp)
    st = ex.stages
    LP, rows = L * P, inp["B"] * inp["Nq"]
    assert rows == 111 and rows % 16 != 0 and (2 * 16) // inp["Nq"] != (2 * 16 + 15) // inp["Nq"]   # a tile spans two images
    # s is unchanged by E (float64 sees sigmoid(30) = 1 - 1e-13 where fp32 sees 1: the samples move by that much)
    assert float((st["s64"] - st["s"]).abs().max()) < 1e-9
    assert float((db.emulate(inp).x_out.double() - ex.x_out).abs().max()) <= float(db.bound(ex).max())
    assert bool((st["x1"] == 0).all()) and torch.equal(st["q2"], inp["qpos"].double())
    aw, gate = st["aw"], st["gate"]
    allowed = {1.0, 0.5, 0.25, 0.0} | ({1.0 / 16} if LP == 16 else set())
    assert set(aw.unique().tolist()) <= allowed and set(aw.unique().tolist()) >= {1.0, 0.5, 0.0}
    single = (aw == 1.0)
    assert bool(single.any(0).any(0).all()), "a point index is never the selected one"
    assert bool((aw > 0)[..., 10:].any()) == (LP > 10)
    # the positions of the points that carry weight: quarter pixels, and every border position on both axes
    for key, sizes in (("h_im", [h for h, _ in inp["shapes"]]), ("w_im", [w for _, w in inp["shapes"]])):
        im = st[key][aw > 0]
        assert bool(((im * 4 - (im * 4).round()).abs() < 1e-9).all())
        size = torch.tensor(sizes).double()[torch.arange(LP) // P].expand_as(st[key])[aw > 0]
        imr = (im * 4).round() / 4
        for edge in (-1.0, -0.5):
            assert bool((imr == edge).any()), (key, edge)
        for back in (1.0, 0.5, 0.0):
            assert bool((imr == size - back).any()), (key, "size -", back)
        assert bool((imr < -2).any()) and bool((imr > size + 1).any())
        frac = imr - imr.floor()
        assert {0.0, 0.25, 0.5, 0.75} <= set(frac.unique().tolist())
    assert float((gate & (aw > 0)).double().mean()) > 0.02
    # the anchors: channels fed by the zero head carry bout alone
    assert bool((inp["value"][:, :, db.M - 1] == 0).all()) and int((inp["bout"] != 0).sum()) == db.D
    vr = inp["vr32"]
    assert set(vr.unique().tolist()) <= {0.5, 0.75, 1.0}
    if L > 1:
        assert bool((vr[:, 0] != vr[:, 1]).any(-1).all()) and bool((vr[0] != vr[1]).any())


@DTYPES
def test_integer_cases_are_exact(dtype):
    lim = db.INT_LIMIT[dtype]
    whole = lambda v: bool((v == v.round()).all())   # noqa: E731
    ex = db.exact(db.oproj_exact(dtype))
    assert whole(ex.stages["t1"]) and float(ex.stages["t1"].abs().max()) <= lim
    pre = ex.inp["attn"].double() @ ex.inp["wo"].double().t() + ex.inp["bo"].double()
    assert bool((pre != pre.to(dtype).double()).any()), "E never moves Wo attn + bo"
    ex = db.exact(db.ffn_exact(dtype))
    rows = ex.inp["x"].shape[0]
    assert rows >= 913 and set(db.rotation(rows).tolist()) == set(range(8))
    for k in ("x2", "h", "y32"):
        assert whole(ex.stages[k]) and float(ex.stages[k].abs().max()) <= lim, k
    h = ex.stages["h"][0].view(8, 256)
    assert all(not torch.equal(h[a], h[b]) for a in range(8) for b in range(a)), "two hidden chunks hold the same values"
    b1 = ex.inp["b1"].double().view(8, 256)
    assert all(bool((b1[a] != b1[b]).all()) for a in range(8) for b in range(a))
    assert bool((ex.x_out == ex.x_out[0]).all())
    ex = db.exact(db.ffn_rounding(dtype))
    y32 = ex.stages["y32"]
    assert whole(y32) and bool((y32 != y32.to(dtype).double()).any()) and float((y32 - 4096).abs().max()) < 200
    ex = db.exact(db.box_exact(dtype))
    for k in ("x3", "r1", "r2"):
        assert whole(ex.stages[k]) and float(ex.stages[k].abs().max()) <= lim, k
    pre = ex.stages["r2"] @ ex.inp["wr3"].double().t() + ex.inp["br3"].double()
    assert bool((pre[:, 3] == lim + 1).all()) and bool((ex.stages["delta"][:, 3] == lim).all())
    assert ex.inp["ref"].double().unique(dim=0).shape[0] == rows_of(ex.inp)


def rows_of(inp):
    return inp["B"] * inp["Nq"]


@DTYPES
def test_float64_gather_is_the_oracles(dtype):
    """the module's float64 gather against oracle/msda_oracle.py's vectorised restatement, on the random case's own projection"""
    import msda_oracle

    for L, P in ((5, 4), (2, 8), (4, 5)):
        inp = db.random_layer(dtype, L, P)
        st = db.exact(inp).stages
        LP, rows, B, Nq = L * P, rows_of(inp), inp["B"], inp["Nq"]
        pj = st["pj"]
        off = pj[:, :16 * LP].view(B, Nq, 8, L, P, 2)
        aw = torch.softmax(pj[:, 16 * LP:24 * LP].view(B, Nq, 8, LP), -1).view(B, Nq, 8, L, P)
        sig = torch.sigmoid(inp["ref"].double()).view(B, Nq, 4)
        vr = inp["vr32"].double()
        box = sig[:, :, None, :] * torch.cat((vr, vr), -1)[:, None]                      # [B, Nq, L, 4]
        loc = box[:, :, None, :, None, :2] + off / P * box[:, :, None, :, None, 2:] * 0.5
        starts, _ = db.level_starts(inp["shapes"])
        want = msda_oracle.msda_forward_numpy(inp["value"].double().numpy(), np.array(inp["shapes"]), np.array(starts),
                                              loc.numpy(), aw.numpy())
        assert np.abs(want.reshape(rows, 256) - st["s64"].numpy()).max() < 1e-12


@DTYPES
def test_pack_then_unpack_is_the_identity(dtype):
    for L, P in ((5, 4), (1, 2), (2, 8)):
        inp = db.random_layer(dtype, L, P)
        back = db.unpack(db.pack(inp), L, P)
        assert set(back) == set(db.weight_shapes(L, P))
        for k, shp in db.weight_shapes(L, P).items():
            assert back[k].shape == shp and back[k].dtype == dtype and torch.equal(back[k], inp[k]), k


def test_supported_table_is_dims_ok():
    """L <= 8, L P even, L P <= 20 -- and the probes and the random case run only (L, P) the entry accepts"""
    table = {(L, P) for L in range(1, 9) for P in range(1, 21) if db.supported(L, P)}
    assert table == {(L, P) for L in range(1, 9) for P in range(1, 21) if (L * P) % 2 == 0 and L * P <= 20}
    assert not db.supported(9, 2) and not db.supported(0, 2) and not db.supported(5, 3) and not db.supported(3, 7)
    assert all(db.supported(L, P) for L, P in db.LP_RANDOM)
    assert {L * P for L, P in db.LP_RANDOM} >= {2, 10, 12, 16, 20}
