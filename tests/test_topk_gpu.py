"""Row-wise top-k kernel (csrc/topk.hip, codetr_topk_*) against torch: the two selections of the detection head
(reference transformer.py:560-561: top 900 of S per-token scores; co_dino_head.py:183-186: top 300 of 900 x 80 sigmoid
scores).  Values must equal torch.topk's exactly (it is a selection, not arithmetic); indices must be the stable
descending order (ties by ascending index), which pins them completely; NaN first as in torch."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _check(x, k):
    from codetr import _cabi, hip_ops

    before = _cabi.CALLS["topk"]
    with torch.no_grad():
        v, i = hip_ops.topk(x, k)
    torch.cuda.synchronize()
    assert _cabi.CALLS["topk"] == before + 1
    # stable descending order of the whole row fixes the indices; every NaN counts as the largest value (torch's
    # documented rule and the CUDA implementation's; torch-ROCm's topk leaves sign-bit NaNs at the bottom)
    xf = x.float()
    nan = torch.isnan(xf)
    xd = xf.double()   # (float64: +-inf map to +-1e300, strictly inside NaN and strictly outside +-finfo(bf16).max)
    key = torch.where(nan, torch.full_like(xd, float("inf")), xd.clamp(min=-1e300, max=1e300))
    order = torch.sort(key, dim=-1, descending=True, stable=True)[1][..., :k]
    assert torch.equal(i, order), "indices are not the stable descending order"
    if not nan.any():
        tv, _ = torch.topk(xf, k, dim=-1)
        assert torch.equal(v.float(), tv), "values differ from torch.topk"
    assert torch.equal(torch.gather(x, -1, i).view(torch.int16), v.view(torch.int16))


@pytest.mark.parametrize("rows,n,k", [(1, 204600, 900), (8, 72000, 300), (2, 30785, 900), (1, 30785, 900), (1, 8193, 300), (1, 77, 50), (3, 1000, 1000), (1, 1024, 1024),
                                      (4, 5000, 1), (2, 77, 50), (1, 1, 1)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_matches_torch_topk(rows, n, k, dtype):
    g = torch.Generator(device=DEV).manual_seed(rows * 1000 + n + k)
    _check(torch.randn(rows, n, device=DEV, generator=g).to(dtype), k)


def test_heavy_ties_like_sigmoid_scores():
    """fp16 sigmoid scores cluster in a few hundred distinct values: thousands of exact ties around the threshold"""
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.sigmoid(torch.randn(4, 72000, device=DEV, generator=g) * 0.05).half()
    assert x.unique().numel() < 400
    _check(x, 300)
    _check(torch.zeros(2, 5000, device=DEV, dtype=torch.float16), 300)           # all equal: indices 0..299
    _check(torch.cat((torch.zeros(1, 100, device=DEV), -torch.zeros(1, 100, device=DEV)), 1).half(), 150)


def test_nan_inf_and_negative_values():
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(2, 4000, device=DEV, generator=g).half()
    x[0, 5] = float("nan")
    x[0, 3000] = float("nan")
    x[0, 17] = float("inf")
    x[1, 9] = float("-inf")
    x[1, 100:200] = -65504.0
    _check(x, 900)
    _check(-x.abs(), 64)


def test_heavy_ties_like_bf16_sigmoid_scores():
    """bf16 keeps 8 significant bits: the head's sigmoid scores take 128 values in [0.5, 1), so the top 300 of 72000
    is a few tie groups, cut in the middle of one"""
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.sigmoid(torch.randn(4, 72000, device=DEV, generator=g) * 2).bfloat16()
    assert x.unique().numel() < 2000 and int((x >= 0.5).float().sum(-1).min()) > 300
    _check(x, 300)
    _check(torch.zeros(2, 5000, device=DEV, dtype=torch.bfloat16), 300)
    _check(torch.cat((torch.zeros(1, 100, device=DEV), -torch.zeros(1, 100, device=DEV)), 1).bfloat16(), 150)


@pytest.mark.parametrize("rows,n", [(2, 30785), (1, 204600)])
def test_encoder_selection_shape_bf16_ties(rows, n):
    """the two-stage selection (top 900 of the per-token scores) on bf16 logits: ties everywhere; the long row goes
    through the chunked entry (codetr_topk_chunked_bf16)"""
    import ctypes

    from codetr import _cabi

    g = torch.Generator(device=DEV).manual_seed(n)
    x = (torch.randn(rows, n, device=DEV, generator=g) * 3).bfloat16()
    assert x.unique().numel() < n // 10
    ws = ctypes.c_int64(0)
    chunks = _cabi.load().codetr_topk_chunks(n, 900, rows, ctypes.cast(ctypes.pointer(ws), ctypes.c_void_p))
    if n == 204600:
        assert chunks > 1, "the long row is expected to take the chunked entry"
    _check(x, 900)
    x[:, ::7] = x[:, :1]        # one large tie group spread over the whole row
    _check(x, 900)


def test_nan_inf_zero_and_extremes_bf16():
    """NaN of both signs first (by index), +inf, finite values, +-0 as equals, -finfo(bf16).max above -inf"""
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(3, 4000, device=DEV, generator=g).to(dt)
    x[0, 5] = float("nan")
    x.view(torch.int16)[0, 3000] = -0x40      # bits 0xffc0: sign-bit NaN
    x[0, 17] = float("inf")
    x[0, 18] = torch.finfo(dt).max
    x[1, 9] = float("-inf")
    x[1, 100:200] = -torch.finfo(dt).max
    x[1, 300:400:2] = -0.0                    # -0 before +0, interleaved: equal values, so ascending index decides
    x[1, 301:400:2] = 0.0
    x[2, :] = -torch.finfo(dt).max
    x[2, 1000:1500] = float("-inf")
    x.view(torch.int16)[2, 3999] = -0x40
    assert torch.isnan(x[0, 3000]) and x[0, 3000].view(torch.int16) < 0
    _check(x, 900)
    _check(-x.abs(), 64)
    _check(x[1:2, 100:400].contiguous(), 300)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_signed_zeros_are_one_value(dtype):
    """-0 == +0: a zero group cut by k keeps its lowest indices, whichever sign comes first"""
    z = torch.zeros(2, 200, device=DEV, dtype=dtype)
    z[0, :100] = -0.0                          # all -0 first, then +0
    z[1, ::2] = -0.0                           # interleaved, -0 at even indices
    assert (z.view(torch.int16) < 0).sum() == 200
    _check(z, 150)
    x = torch.cat((-torch.ones(2, 50, device=DEV), z.float(), torch.ones(2, 50, device=DEV)), 1).to(dtype)
    _check(x, 120)                             # 50 ones, then 70 of the zero group in index order


def test_unsupported_falls_back_to_torch():
    from codetr import _cabi, hip_ops

    x = torch.randn(2, 5000, device=DEV)
    before = _cabi.CALLS["topk"]
    v, i = hip_ops.topk(x, 10)                      # fp32: library path
    assert _cabi.CALLS["topk"] == before
    tv, ti = torch.topk(x, 10, dim=-1)
    assert torch.equal(v, tv) and torch.equal(i, ti)
    with torch.no_grad():
        v, i = hip_ops.topk(x.half(), 2000)         # k > 1024: library path
    assert _cabi.CALLS["topk"] == before and v.shape == (2, 2000)
