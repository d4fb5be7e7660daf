"""The native 16-bit ResNet-50 backbone: its kernels (codetr_conv_tokens_*, act 3 of codetr_linear_*, the stem's window
gather, the token-major max pool) against PyTorch, and the R50 Co-DINO model on the token route against the fp32
oracle, the steady-state kernel whitelist and the plan runner.

Kernel tolerance (as tests/test_linear_gpu.py): the 16-bit inputs are exact, the reference sums in fp64, the kernel in
fp32 with one rounding at the store: |err| <= 1 ulp |y| + K 2^-22 (+ 1 ulp of the pre-residual value where a residual
is added to the rounded result)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import codetr_fp32 as M
import fullsize_cases as FC
from conftest import ROOT
from helpers_model import assert_close_lowp, check_16bit_detections, seeded_params, valid_topk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_UNSUPPORTED = -4
RUNNER = os.path.join(ROOT, "runner", "codetr_runner")
LIB = os.path.join(ROOT, "co-detr-tensorrt_amd", "codetr", "libcodetr_hip.so")


def _g(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ulp(dtype):
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7


def _conv_ref(x4d, w, b, k, stride, pad, act, r):
    """fp64 F.conv2d on the same 16-bit values -> (pre-residual value, final value) as [B, Ho, Wo, Cout]"""
    y = F.conv2d(x4d.double().permute(0, 3, 1, 2), w.double(), None, stride, pad).permute(0, 2, 3, 1)
    if b is not None:
        y = y + b.double()
    pre = y
    if act == "relu":
        y = torch.relu(y)
    if r is not None:
        y = y + r.double()
    if act == "relu_res":
        y = torch.relu(y)
    return pre, y


# (C, Cout, k, stride): the R50's 3x3 convs (stride 1 and the stride-2 first blocks) and its stride-2 1x1 downsamples
CONV_CASES = [(64, 64, 3, 1), (128, 128, 3, 2), (256, 256, 3, 1), (512, 512, 3, 2),
              (256, 512, 1, 2), (512, 1024, 1, 2), (1024, 2048, 1, 2), (128, 128, 3, 1)]
MAPS = [(25, 33), (13, 17), (1, 1), (2, 3)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("C,Cout,k,stride", CONV_CASES)
def test_conv_tokens_vs_conv2d(C, Cout, k, stride, dtype):
    from codetr import hip_ops

    pad = k // 2
    g = _g(C + Cout + k + stride)
    epilogues = [(False, None, False), (True, "relu", False), (True, None, True), (True, "relu_res", True),
                 (False, "relu_res", True)]
    for mi, (H, W) in enumerate(MAPS):
        bias, act, res = epilogues[(mi + C // 64 + k + stride) % len(epilogues)]
        x = torch.randn(2, H, W, C, device=DEV, generator=g).to(dtype)
        w = (torch.randn(Cout, C, k, k, device=DEV, generator=g) / (k * k * C) ** 0.5).to(dtype)
        b = torch.randn(Cout, device=DEV, generator=g).to(dtype) if bias else None
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        r = torch.randn(2, Ho, Wo, Cout, device=DEV, generator=g).to(dtype) if res else None
        wk = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
        y = hip_ops.conv_tokens(x, wk, b, k, stride, pad, act=act, residual=r)
        torch.cuda.synchronize()
        pre, ref = _conv_ref(x, w, b, k, stride, pad, act, r)
        assert y.shape == (2, Ho, Wo, Cout) and y.dtype == dtype
        u = _ulp(dtype)
        tol = u * ref.abs() + k * k * C * 2.0 ** -22 + 1e-3 * u
        if r is not None:
            tol = tol + u * pre.abs()
        err = (y.double() - ref).abs()
        bad = err > tol
        assert not bad.any(), (f"{(H, W)} bias={bias} act={act} res={res}: {int(bad.sum())} / {bad.numel()} outside "
                               f"the bound; max err {err.max().item():.3e}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_conv_tokens_matches_im2col_baseline_bit_for_bit_shape_and_domain(dtype):
    """the A/B baseline (im2col + linear) computes the same sums; domain violations are CODETR_E_UNSUPPORTED"""
    from codetr import _cabi, hip_ops

    g = _g(5)
    x = torch.randn(2, 19, 23, 128, device=DEV, generator=g).to(dtype)
    w = (torch.randn(128, 9 * 128, device=DEV, generator=g) / 34.0).to(dtype)
    b = torch.randn(128, device=DEV, generator=g).to(dtype)
    before = _cabi.CALLS["conv_tokens"]
    y = hip_ops.conv_tokens(x, w, b, 3, 2, 1, act="relu")
    assert _cabi.CALLS["conv_tokens"] == before + 1
    hip_ops.R50_CONV_IM2COL = True
    try:
        y2 = hip_ops.conv_tokens(x, w, b, 3, 2, 1, act="relu")
    finally:
        hip_ops.R50_CONV_IM2COL = False
    assert _cabi.CALLS["conv_tokens"] == before + 1
    u = _ulp(dtype)
    assert ((y.float() - y2.float()).abs() <= 2 * u * y2.float().abs() + 1e-3).all()

    lib = _cabi.load()
    fn = lib.codetr_conv_tokens_f16 if dtype == torch.float16 else lib.codetr_conv_tokens_bf16
    out = torch.empty(2 * 19 * 23 * 256, dtype=dtype, device=DEV)
    xs = torch.zeros(2 * 19 * 23 * 128, dtype=dtype, device=DEV)
    ws = torch.zeros(256 * 9 * 128, dtype=dtype, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    base = dict(B=2, H=19, W=23, C=128, Cout=128, k=3, stride=1, pad=1, act=0)

    def call(**kw):
        a = dict(base, **kw)
        return fn(s, xs.data_ptr(), ws.data_ptr(), None, None, out.data_ptr(), a["B"], a["H"], a["W"], a["C"],
                  a["Cout"], a["k"], a["stride"], a["pad"], a["act"])

    assert call() == 0
    for bad in (dict(C=96), dict(C=32), dict(Cout=12), dict(k=5, pad=2), dict(k=7, pad=3), dict(stride=3),
                dict(pad=3), dict(act=4)):
        assert call(**bad) == E_UNSUPPORTED, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("variant,M,N,K", [("tile128", 1000, 256, 512), ("tile256", 12800, 1024, 256),
                                           ("xs", 33000, 256, 256)])
def test_linear_act3_relu_after_residual(variant, M, N, K, dtype):
    from codetr import _cabi, hip_ops

    assert _cabi.linear_variant(M, N, K, "relu_res", True) == variant
    g = _g(M + N)
    x = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(dtype)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    r = torch.randn(M, N, device=DEV, generator=g).to(dtype)
    before = dict(_cabi.CALLS)
    y = hip_ops.linear(x, w, b, act="relu_res", residual=r)
    torch.cuda.synchronize()
    assert _cabi.CALLS["linear_" + variant] == before["linear_" + variant] + 1
    assert _cabi.CALLS["linear_sk"] == before["linear_sk"] and _cabi.CALLS["linear_pp"] == before["linear_pp"]
    pre = x.double() @ w.double().t() + b.double()
    ref = torch.relu(pre + r.double())
    u = _ulp(dtype)
    err = (y.double() - ref).abs()
    bad = err > u * ref.abs() + u * pre.abs() + K * 2.0 ** -22 + 1e-3 * u
    assert not bad.any(), f"{int(bad.sum())} outside the bound, max err {err.max().item():.3e}"
    assert (y >= 0).all()
    # exactly act 0 + residual, then the ReLU
    y0 = hip_ops.linear(x, w, b, residual=r)
    assert torch.equal(y, torch.relu(y0))
    # no residual: act 3 is act 1
    assert torch.equal(hip_ops.linear(x, w, b, act="relu_res"), hip_ops.linear(x, w, b, act="relu"))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("H,W", [(37, 45), (8, 8), (1, 1), (5, 2)])
def test_stem_gather_vs_unfold(H, W, dtype):
    from codetr import _cabi

    x = torch.randn(2, 3, H, W, device=DEV, generator=_g(H * W)).to(dtype)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    cols = torch.full((2 * Ho * Wo, 192), 7.0, dtype=dtype, device=DEV)
    _cabi.conv_im2col_nchw(x, 7, 2, 3, 192, cols)
    ref = F.unfold(x.float(), 7, padding=3, stride=2).transpose(1, 2).reshape(-1, 147).to(dtype)
    assert torch.equal(cols[:, :147], ref)
    assert (cols[:, 147:] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("H,W", [(37, 45), (16, 16), (1, 1), (2, 3), (7, 1)])
def test_maxpool_tokens_vs_max_pool2d(H, W, dtype):
    from codetr import hip_ops

    g = _g(H + W)
    x = torch.randn(2, H, W, 64, device=DEV, generator=g).to(dtype)
    special = torch.rand(x.shape, device=DEV, generator=g)
    x[special < 0.02] = float("nan")
    x[(special >= 0.02) & (special < 0.04)] = float("inf")
    x[(special >= 0.04) & (special < 0.08)] = float("-inf")
    x[0, :, :, :8] = float("-inf")           # windows of -inf only: the result is -inf, padding never wins
    y = hip_ops.maxpool_tokens(x)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2).float(), 3, 2, 1).permute(0, 2, 3, 1).to(dtype)
    assert y.shape == ref.shape == (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    assert torch.equal(y.isnan(), ref.isnan())
    fin = ~ref.isnan()
    assert torch.equal(y[fin], ref[fin])
    assert torch.equal(y[fin].view(torch.int16), ref[fin].view(torch.int16))


# ---- the model ---------------------------------------------------------------------------------------------------


def _tiny_r50(seed=77, scale=1.0):
    import codetr
    from test_model_gpu import _tiny_codetr_cfg

    torch.manual_seed(0)
    model = codetr.CoDETR(**_tiny_codetr_cfg("r50"))
    model.init_weights()
    spec = [(k, tuple(v.shape)) for k, v in model.named_parameters()]
    full = dict(model.state_dict())
    full.update(seeded_params(spec, seed, scale=scale))
    for k in full:
        if k.endswith("running_var"):
            full[k] = torch.rand(full[k].shape) + 0.5
        elif k.endswith("running_mean"):
            full[k] = torch.randn(full[k].shape) * 0.1
    model.load_state_dict(full)
    return model, full


def _inputs(H, W, B=2):
    g = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, H, W, generator=g)
    mask = torch.zeros(B, H, W)
    mask[-1, :, int(W * 0.8):] = 1
    mask[-1, int(H * 0.9):, :] = 1
    return img, mask


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hw", [(96, 128), (100, 132)])
def test_tiny_r50_16bit_token_route_vs_oracle(hw, dtype):
    from codetr import _cabi

    model, full = _tiny_r50()
    model = model.to(DEV).to(dtype).eval()
    H, W = hw
    img, mask = _inputs(H, W)
    cap_o = {}
    M.codetr_forward(full, img, mask, backbone="r50", num_query=50, max_per_img=20, capture=cap_o)
    picks = valid_topk(cap_o["enc_outputs_class"], cap_o["enc_outputs_coord_unact"], 50)
    M.codetr_forward(full, img, mask, backbone="r50", num_query=50, max_per_img=20, forced_topk=picks, capture=cap_o)
    cap = {}
    before = dict(_cabi.CALLS)
    with torch.no_grad():
        boxes, scores, labels = model(img.to(DEV).to(dtype), mask.to(DEV).to(dtype),
                                      forced_topk_indices=cap_o["topk_indices"].to(DEV), capture=cap)
    torch.cuda.synchronize()
    assert cap["route"] == "tokens"
    assert _cabi.CALLS["conv_tokens"] - before["conv_tokens"] == 16 + 3     # 16 3x3 convs + 3 strided downsamples
    assert _cabi.CALLS["maxpool_tokens"] - before["maxpool_tokens"] == 1
    assert _cabi.CALLS["conv_im2col_nchw"] - before["conv_im2col_nchw"] == 1
    rel = 1e-2 if dtype == torch.float16 else 6e-2
    for i, (a, b) in enumerate(zip(cap["backbone_feats"], cap_o["backbone_feats"])):
        assert_close_lowp(a.float().cpu().numpy(), b.numpy(), rel, None, f"backbone level {i}")
    for i, (a, b) in enumerate(zip(cap["neck_feats"], cap_o["neck_feats"])):
        assert_close_lowp(a.float().cpu().numpy(), b.numpy(), rel, None, f"neck level {i}")
    assert_close_lowp(cap["memory"].float().cpu().numpy(), cap_o["memory"].numpy(), rel, None, "encoder memory")
    assert_close_lowp(cap["outputs_classes"].float().cpu().numpy(), cap_o["outputs_classes"].numpy(), 2.5 * rel, None,
                      "class logits")
    assert boxes.shape == (2, 20, 4) and scores.shape == (2, 20) and labels.dtype == torch.int64
    # the detections against float64 re-derived from the product's own logits and coordinates (sigmoid -> topk ->
    # decode_boxes at the kernels' rounding; see helpers_model.check_16bit_detections)
    check_16bit_detections((boxes, scores, labels), cap, H, W)


def test_tiny_r50_fp32_keeps_the_nchw_route_bit_for_bit():
    from codetr import _cabi, hip_ops

    model, _ = _tiny_r50()
    model = model.to(DEV).eval()
    img, mask = _inputs(96, 128)
    img, mask = img.to(DEV), mask.to(DEV)
    outs = []
    # MIOpen's default fp32 convolutions differ in the last bits between a first and a later call (either switch
    # setting): deterministic algorithms make the two runs comparable bit for bit
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for native in (True, False):
            hip_ops.R50_NATIVE = native
            cap = {}
            before = _cabi.CALLS["conv_tokens"]
            with torch.no_grad():
                outs.append(model(img, mask, capture=cap))
            torch.cuda.synchronize()
            assert cap["route"] == "nchw" and _cabi.CALLS["conv_tokens"] == before
    finally:
        hip_ops.R50_NATIVE = True
        torch.backends.cudnn.deterministic = det
    for a, b in zip(*outs):   # (random weights: a padded image's boxes can hold NaN, on both sides alike)
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=12345.0), b.nan_to_num(nan=12345.0))


def test_r50_native_switch_off_gives_the_nchw_route_in_fp16():
    from codetr import hip_ops

    model, _ = _tiny_r50()
    model = model.to(DEV).half().eval()
    img, mask = _inputs(96, 128)
    hip_ops.R50_NATIVE = False
    try:
        assert hip_ops.nondefault_switches() == ["R50_NATIVE"]
        cap = {}
        with torch.no_grad():
            model(img.to(DEV).half(), mask.to(DEV).half(), capture=cap)
    finally:
        hip_ops.R50_NATIVE = True
    assert cap["route"] == "nchw"


def test_r50_608_fp16_vs_oracle_fixture():
    """BASELINE config 1 (Co-DINO R50, 608x608) in fp16 on the native route against the committed oracle rows"""
    from codetr import _cabi

    name = "r50_608"
    fx = FC.load_fixture(name)
    model, full, img, mask = FC.build_case(name)
    assert str(fx["spec_digest"]) == FC.spec_digest(full), "fixture was made for another parameter layout: regenerate"
    model = model.to(DEV).half().eval()
    cap = {}
    before = dict(_cabi.CALLS)
    with torch.no_grad():
        boxes, scores, labels = model(img.to(DEV).half(), mask.to(DEV).half(),
                                      forced_topk_indices=torch.from_numpy(fx["topk_indices"]).to(DEV), capture=cap)
    torch.cuda.synchronize()
    assert cap["route"] == "tokens"
    assert _cabi.CALLS["conv_tokens"] - before["conv_tokens"] == 19
    got = FC.sample_capture(name, cap)
    deep = {"final_state": 2.5, "outputs_classes": 2.5}
    for k, v in got.items():
        assert_close_lowp(v, fx[k], 1e-2 * deep.get(k, 1.0), None, f"{name}: {k}")
    np.testing.assert_allclose(scores.float().cpu().numpy(), fx["scores"], rtol=2e-2, atol=2e-3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_r50_steady_state_forward_issues_only_native_kernels(dtype):
    from codetr.export import is_own_kernel

    model, _ = _tiny_r50(seed=5, scale=1.0)
    model = model.to(DEV).to(dtype).eval()
    img, mask = _inputs(160, 192)
    img, mask = img.to(DEV).to(dtype), mask.to(DEV).to(dtype)
    with torch.no_grad():
        for _ in range(2):
            model(img, mask)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            model(img, mask)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if "Memcpy" not in n and "Memset" not in n]
    assert len(kernels) > 100, "the profiler saw no kernels"
    foreign = sorted({n[:120] for n in kernels if not is_own_kernel(n)})
    assert not foreign, f"device work outside libcodetr_hip.so on the steady-state R50 {dtype} forward: {foreign}"
    assert not [n for n in names if "Memcpy" in n], "a device copy on the steady-state R50 forward"


def test_r50_fp16_plan_replays_in_the_runner(tmp_path):
    from codetr.export import export_plan

    model, _ = _tiny_r50(seed=5, scale=1.0)
    model = model.to(DEV).half().eval()
    img, mask = _inputs(160, 192)
    img, mask = img.to(DEV).half(), mask.to(DEV).half()
    plan = str(tmp_path / "r50.plan")
    info = export_plan(model, img, mask, plan)
    assert info["launches"] > 100
    with torch.no_grad():
        boxes, scores, labels = model(img, mask)
    torch.cuda.synchronize()
    for extra in ([], ["--no-graph"]):
        out = tmp_path / ("out" + "_".join(extra))
        out.mkdir()
        p = subprocess.run([RUNNER, "--plan", plan, "--lib", LIB, "--iters", "3", "--out-dir", str(out)] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        rep = json.loads(p.stdout.strip().splitlines()[-1])
        assert rep["launches"] == info["launches"] and rep["hipgraph"] == (not extra)
        b = np.fromfile(os.path.join(out, "boxes.bin"), dtype=np.float16)
        s = np.fromfile(os.path.join(out, "scores.bin"), dtype=np.float16)
        lab = np.fromfile(os.path.join(out, "labels.bin"), dtype=np.int64)
        assert np.array_equal(b.view(np.uint16), boxes.cpu().numpy().reshape(-1).view(np.uint16))
        assert np.array_equal(s.view(np.uint16), scores.cpu().numpy().reshape(-1).view(np.uint16))
        assert np.array_equal(lab, labels.cpu().numpy().reshape(-1))
