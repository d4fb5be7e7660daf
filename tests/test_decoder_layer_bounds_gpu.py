"""codetr_decoder_layer_{f16,bf16} (csrc/decoder_layer.hip) through _cabi.decoder_layer on the cases of
tests/decoder_layer_bounds.py: exact gathers at every (L, P) family, exact out-projection / FFN routing / box refinement, the
sine embedding against float64, the random layer against float64 and the fp32 emulation; the library's own (L, P) table; guard
rows behind a partial last tile; row locality under a NaN row."""
import pytest
import torch

import decoder_layer_bounds as db

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def _kernel(inp):
    return db.valid_rows(db.run_kernel(inp), inp["B"] * inp["Nq"])


@DTYPES
@pytest.mark.parametrize("name", db.CASE_NAMES)
def test_kernel_passes_the_case(name, dtype):
    from codetr import _cabi

    before = _cabi.CALLS["decoder_layer"]
    fig = db.hold(name, dtype, _kernel, DEV)
    assert _cabi.CALLS["decoder_layer"] > before
    print(f"{name} {dtype}: {fig}")


def test_library_table_is_the_modules():
    from codetr import _cabi

    for L in range(1, 9):
        for P in range(1, 21):
            assert _cabi.decoder_layer_supported(256, 8, L, P, 2048, 4, 128) == db.supported(L, P), (L, P)
    assert not _cabi.decoder_layer_supported(256, 8, 9, 2, 2048, 4, 128)


def _bits(t):
    return t.contiguous().view(torch.int16)


@DTYPES
@pytest.mark.parametrize("Nq", [11, 7, 21], ids=["rows33", "rows21", "rows63"])
@pytest.mark.parametrize("form", ["tail_head", "tail", "head"])
def test_guard_rows_stay_intact(form, Nq, dtype):
    """rows % 16 in {1, 5, 15}: every output has 16 rows of a sentinel behind `rows`, every input is exactly `rows` long; the
    sentinels keep their bits and the valid rows are those of a launch without guard rows"""
    inp = db.random_layer(dtype, 5, 4, B=3, Nq=Nq, head=form != "tail")
    inp["tail"] = form != "head"
    inp = db.to_device(inp, DEV)
    rows = 3 * Nq
    assert rows % 16 in (1, 5, 15)
    blobs = db.pack(inp, DEV)
    plain = db.run_kernel(inp, blobs)
    guarded = db.run_kernel(inp, blobs, guard=16, sentinel=-7.0)
    want = _bits(torch.tensor([-7.0], dtype=dtype, device=DEV))
    for k in db.outputs_of(inp):
        g, p = getattr(guarded, k), getattr(plain, k)
        assert g.shape[0] == rows + 16 and bool((_bits(g[rows:]) == want).all()), f"{k}: a sentinel row was written"
        assert torch.equal(_bits(g[:rows]), _bits(p)), k
        assert bool(torch.isfinite(p.float()).all()), k


@DTYPES
@pytest.mark.parametrize("row", [40, 110], ids=["mid_tile", "last_valid_row"])
def test_a_nan_row_stays_in_its_row(row, dtype):
    """x, attn, qpos and ref of one row are NaN: every other row of every output keeps its bits (111 rows: row 40 sits in the
    middle of a tile, row 110 is the last valid row of the partial tile, the one the clamped rows behind it reload)"""
    inp = db.to_device(db.random_layer(dtype, 5, 4), DEV)
    assert inp["x"].shape[0] == 111
    blobs = db.pack(inp, DEV)
    clean = db.run_kernel(inp, blobs)
    bad = dict(inp)
    for k in ("x", "attn", "qpos", "ref"):
        bad[k] = inp[k].clone()
        bad[k][row] = float("nan")
    dirty = db.run_kernel(bad, blobs)
    keep = torch.arange(111, device=DEV) != row
    for k in db.outputs_of(inp):
        c, d = getattr(clean, k), getattr(dirty, k)
        assert torch.equal(_bits(c[keep]), _bits(d[keep])), f"{k}: a NaN row reached another row"
    assert bool(torch.isnan(dirty.x_out[row].float()).all())          # (the ReLUs of the HEAD turn a NaN into 0: fmaxf)
