"""CPU: the host contract of the linear / convolution launchers (csrc/gemm_f16.hip, gemm_tile128.hip, gemm_tile256.hip,
gemm_xs.hip) against tests/golden/linear_host_contract.json, the answers of the library BEFORE those launchers were
last moved (tests/golden/make_linear_host_contract.py wrote it).

Callers tell E_UNSUPPORTED (try another route) apart from E_BADARG, so a launcher's checks keep their order and their
codes.  A rejected call returns before any HIP call, as tests/test_cabi.py relies on, so every row runs here; the two
queries are pure functions of their arguments.
"""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_linear_host_contract", os.path.join(GOLDEN, "make_linear_host_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib(gen):
    from codetr import _cabi

    return gen.bind(_cabi.LIB_PATH)


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "linear_host_contract.json")) as f:
        return json.load(f)


def test_rejected_calls_return_the_recorded_codes(gen, lib, table):
    from codetr import _cabi

    wrong = []
    for entry, args, code in table["rows"]:
        assert code < 0   # a row the library accepts would launch a kernel
        for name in gen.entries(entry):
            rc = gen.call(lib, name, args)
            if rc != code:
                wrong.append((name, args, code, rc))
    assert not wrong, wrong[:10]
    stems = {entry for entry, _, _ in table["rows"]}
    assert stems == {"codetr_linear_*", "codetr_linear_bf16_f16out", "codetr_linear_xadd_*", "codetr_linear_ln_*",
                     "codetr_linear_splitk_*", "codetr_conv_tokens_*", "codetr_encoder_projections_*",
                     "codetr_encoder_projections_posgen_*"}
    # the three codes, by the header's names
    assert {code for _, _, code in table["rows"]} == {-1, -3, _cabi.E_UNSUPPORTED}


def test_variant_and_splitk_plan_over_the_grid(gen, lib, table):
    q = table["queries"]
    assert (q["M"], tuple(q["acts"]), tuple(q["head_dims"]), q["letters"]) == (gen.GRID_M, gen.ACTS, gen.HEAD_DIMS, gen.LETTER)
    assert sorted(q["grid"]) == sorted(f"{N},{K}" for N in gen.GRID_N for K in gen.GRID_K)
    assert q["M"][0] == 1 and q["M"][-1] > 614400
    for key, want in q["grid"].items():
        N, K = map(int, key.split(","))
        assert gen.variant_letters(lib, N, K, q["M"]) == want["variant"], key
        assert [gen.plan(lib, M, N, K) for M in q["M"]] == want["plan"], key
    for M, N, K, letters, plan in q["named"]:
        assert gen.variant_letters(lib, N, K, [M]) == letters and gen.plan(lib, M, N, K) == plan, (M, N, K)


def test_table_agrees_with_the_shapes_the_gpu_tests_name(table):
    """tests/test_linear_gpu.py::test_linear_splitk_plan_and_row_mask states these plans; the table holds the same"""
    named = {(M, N, K): (letters, plan) for M, N, K, letters, plan in table["queries"]["named"]}
    assert named[(204600, 256, 2048)][1] == [1, 0] and named[(900, 256, 256)][1] == [1, 0]
    assert named[(1444, 768, 3072)][1][0] == 3 and named[(2048, 1024, 4096)][1][0] == 2
    assert named[(2176, 1024, 4096)][1] == [1, 0]
    splits, nbytes = named[(300, 64, 2048)][1]
    assert splits >= 2 and nbytes == splits * 300 * 64 * 4
    # every kernel behind codetr_linear_* and the refusal appear in the grid
    seen = set("".join(v["variant"] for v in table["queries"]["grid"].values()))
    assert seen == set(table["queries"]["letters"].values()) - {"u"}   # (every K of the grid is a multiple of 64)
