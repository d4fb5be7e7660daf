"""Functional compute layer of the host package: every tensor op the model modules need goes
through one of these functions, so that "which kernel runs" is decided in exactly one place.

GPU-only by design.  MSDA always runs the hand-written HIP kernel (C ABI).  The dense ops
(linear / layer-norm / window attention / ...) run the hand-written kernels of libcodetr_hip.so
where they exist (``NATIVE`` lists them) and PyTorch-ROCm library kernels otherwise -- PyTorch
here is plumbing (rocBLAS / hipBLASLt / MIOpen behind ATen), used until the native kernel for
that op lands, never as a fallback for a native kernel that exists.

There is no CPU path: a CPU tensor reaching any of these functions is an error (the CPU
formulation of the model lives in oracle/ and is test infrastructure).
"""

import collections
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _appearance, _assign, _cabi, _jpeg, _jpeg_dec, _motion, _redact, _wbf

# ops served by hand-written HIP kernels in this build (kept in sync with include/codetr_hip.h)
NATIVE = {"msda", "linear(f16/bf16, K%64==0)", "layer_norm(f16/bf16)", "swin_window_attention(f16, head_dim 32)",
          "msda_fused(softmax + sampling locations in-kernel)", "groupnorm_tokens(f16, 8 ch/group)",
          "sine_pos_tokens(f16, + level_embed)", "ffn_fused(f16, 256 -> hidden -> 256, ReLU, + identity)",
          "mask_pyramid(level masks + running valid counts + valid ratios)",
          "query_sine_embed(f16: sigmoid x valid ratios + sine embedding of the decoder reference boxes)",
          "encoder_geometry(f16: reference points, proposals, keep/drop state)", "row_max(f16)",
          "preprocess_image(u8 -> f16/f32, cv2-exact resize + pad + normalise + mask)", "batched_nms(f32)",
          "preprocess_batch(u8 -> f16/bf16/f32, <= 32 images of any size per launch, stacked + padded)",
          "postprocess_detections(f16/bf16/f32: threshold + sort + per-class NMS + rescale, one workgroup per image)",
          "postprocess_detections_soft(f16/bf16/f32: threshold + per-class soft-NMS (linear / naive) + max_per_img + rescale)",
          "patch_merge_layernorm(f16: Swin 2x2 gather + LayerNorm)",
          "msda_encoder_packed(f16/bf16: LDS-staged gather for the encoder's self-attention, csrc/msda_encoder4.hip)",
          "patch_embed(f16/bf16: 4x4 patch gather + GEMM)",
          "mha_attention(f16/bf16: dense softmax attention, head_dim 32, <= 1024 keys)",
          "topk(f16/bf16 rows, k <= 1024: radix select + bitonic sort)",
          "im2col_tokens(16-bit token-major maps)",
          "resnet50(f16/bf16: implicit-GEMM conv_tokens, stem window gather + GEMM, maxpool_tokens, BN folded)",
          "small_ops(f16: add, sigmoid, gather_rows, decode_boxes, valid_ratios)",
          "linear_fp8(e4m3 x e4m3, K%128==0) + layer_norm_fp8 + cast_fp8", "ffn_fp8(fused FFN, both products e4m3)"}


# bench.py sets this to a list to time every native linear launch with HIP events on its launch stream
# (entries: (start_event, end_event, flops, M, N, K)); None in normal operation
LINEAR_PROFILE = None
# same hook for the other two heavy kernels: dict name -> list of (start_event, end_event, meta dict); None normally
KERNEL_PROFILE = None


def _timed(name, meta, launch, device):
    """run `launch()`; when bench.py has armed KERNEL_PROFILE, bracket it with HIP events on the launch stream"""
    if KERNEL_PROFILE is None:
        return launch()
    st = torch.cuda.current_stream(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    r = launch()
    e1.record(st)
    KERNEL_PROFILE.setdefault(name, []).append((e0, e1, meta))
    return r


def _timed_linear(launch, device, M, N, K, *tag):
    """run `launch()`; when bench.py has armed LINEAR_PROFILE, bracket it with HIP events on the launch stream and append
    (start, end, flops, M, N, K, *tag) -- unless launch() returned False: a launch the library did not accept"""
    if LINEAR_PROFILE is None:
        return launch()
    st = torch.cuda.current_stream(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    r = launch()
    e1.record(st)
    if r is not False:
        LINEAR_PROFILE.append((e0, e1, 2.0 * M * N * K, M, N, K) + tag)
    return r


def _gpu(x, what):
    if not x.is_cuda:
        raise RuntimeError(
            f"codetr.hip_ops.{what}: got a {x.device.type} tensor; this package computes on MI355X only "
            "(the CPU formulation is the oracle in oracle/, not a fallback)"
        )


LINEAR_PP = True     # route switch (A/B): False keeps the long-K layers on the round-4 kernels


def _persistent_ok(mk, head_major, out, x2, w, r2, bias):
    """what both persistent GEMMs ask of their operands: no row mask / head-major output, 16-byte aligned bases"""
    return (mk is None and not head_major and out.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0
            and w.data_ptr() % 16 == 0 and (r2 is None or r2.data_ptr() % 16 == 0)
            and (bias is None or bias.data_ptr() % 16 == 0))


def linear(x, weight, bias=None, act=None, residual=None, row_mask=None, head_major=None):
    """y = act(x @ weight.T + bias) (+ residual);  act in {None, 'relu', 'gelu', 'relu_res'}.
    'relu_res': y = relu(x @ weight.T + bias + residual) -- the ReLU after the residual of a ResNet bottleneck.
    row_mask (bool, x.shape[:-1]): rows where it is True come out as zeros (before the residual).
    head_major = head_dim: x must be [B, S, K]; the result is returned as [B, N/head_dim, S, head_dim] (each head's
    map contiguous) instead of [B, S, N] -- the value-map layout of the head-major MSDA kernel (native path only)."""
    _gpu(x, "linear")
    if _cabi.linear_supported(x, weight):
        # hand-written MFMA GEMM with the bias / activation / residual folded into its epilogue
        K = x.shape[-1]
        N = weight.shape[0]
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        w = weight if weight.is_contiguous() else weight.contiguous()
        r2 = None
        if residual is not None:
            r2 = residual.reshape(-1, N)
            if not r2.is_contiguous():
                r2 = r2.contiguous()
        mk = None
        if row_mask is not None:
            mk = row_mask.reshape(-1)
            if mk.dtype != torch.bool and mk.dtype != torch.uint8:
                mk = mk != 0
            mk = mk.contiguous()
        hm_rows = hm_hd = 0
        if head_major:
            if x.dim() != 3 or residual is not None:
                raise ValueError("head_major needs a [B, S, K] input and no residual")
            hm_rows, hm_hd = x.shape[1], int(head_major)
        out = torch.empty((x2.shape[0], N), dtype=x.dtype, device=x.device)
        if x2.shape[0] > 0:
            with torch.cuda.device(x.device):
                # act 'relu_res' exists on codetr_linear_* only: the split-K and persistent GEMMs reject it
                res_act = act == "relu_res"
                splits, ws_bytes = (1, 0) if (head_major or res_act) else _cabi.linear_splitk_plan(x2.shape[0], N, K)
                if res_act:
                    launch = lambda: _cabi.linear(x2, w, bias, r2, act, out, mk, hm_rows, hm_hd)  # noqa: E731
                elif splits > 1:
                    # few output tiles, long K (the neck's extra level as a GEMM): two-pass split-K, fp32 partials
                    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
                    launch = lambda: _cabi.linear_splitk(x2, w, bias, r2, act, out, splits, ws, mk)  # noqa: E731
                elif (LINEAR_PP and _persistent_ok(mk, head_major, out, x2, w, r2, bias)
                      and _cabi.linear_pp_preferred(x2.shape[0], N, K, act, r2 is not None)):
                    # the long-K layers with a tile per CU (Swin stages 2-3, stage 1's fc2): ping-pong persistent GEMM
                    launch = lambda: _cabi.linear_pp(x2, w, bias, r2, act, out)  # noqa: E731
                elif (_persistent_ok(mk, head_major, out, x2, w, r2, bias)
                      and _cabi.linear_sk_preferred(x2.shape[0], N, K, act, r2 is not None)):
                    # the large short-K layers (Swin stages 0-2, the encoder's output projections): persistent GEMM
                    launch = lambda: _cabi.linear_sk(x2, w, bias, r2, act, out)  # noqa: E731
                else:
                    launch = lambda: _cabi.linear(x2, w, bias, r2, act, out, mk, hm_rows, hm_hd)  # noqa: E731
                _timed_linear(launch, x.device, x2.shape[0], N, K)
        if head_major:
            return out.view(x.shape[0], N // hm_hd, hm_rows, hm_hd)
        return out.view(*x.shape[:-1], N)
    if head_major:
        raise RuntimeError("head_major output exists only on the native linear (f16/bf16, K % 64 == 0)")
    # fp32 / odd-K layers (patch-embed is a conv; fp32 runs are parity runs): ATen library GEMM
    y = F.linear(x, weight, bias)
    if act == "relu_res":
        if row_mask is not None:
            y = y.masked_fill(row_mask[..., None], 0.0)
        return F.relu(y + residual if residual is not None else y)
    if act == "relu":
        y = F.relu(y, inplace=True)
    elif act == "gelu":
        y = F.gelu(y)
    elif act is not None:
        raise ValueError(act)
    if row_mask is not None:
        y = y.masked_fill(row_mask[..., None], 0.0)
    if residual is not None:
        y = y + residual
    return y


LN_GEMM = True   # route switch (tools/ab_host_routes.py patches it): False = LayerNorm as its own kernel in front of the GEMM


def linear_ln_supported(x, norm_weight, weight):
    """True when LayerNorm(x) @ weight.T runs as ONE kernel (the norm applied in the short-K GEMM's operand load)"""
    return (LN_GEMM and x.is_cuda and norm_weight is not None and norm_weight.dtype == x.dtype and weight.dtype == x.dtype
            and not torch.is_grad_enabled() and norm_weight.shape[0] == x.shape[-1]
            and _cabi.linear_xadd_supported(x.numel() // max(x.shape[-1], 1), weight.shape[0], x.shape[-1], x.dtype))


def linear_ln(x, norm_weight, norm_bias, eps, weight, bias=None, act=None):
    """act(LayerNorm(x) @ weight.T + bias): Swin's norm1 -> qkv and norm2 -> fc1 (reference swin.py:345-386), where only
    the GEMM reads the normalised rows.  Falls back to layer_norm + linear where the fused form does not apply."""
    _gpu(x, "linear_ln")
    if linear_ln_supported(x, norm_weight, weight):
        K, N = x.shape[-1], weight.shape[0]
        x2 = x.reshape(-1, K)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        w = weight if weight.is_contiguous() else weight.contiguous()
        out = torch.empty((x2.shape[0], N), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            ok = _timed_linear(lambda: _cabi.linear_ln(x2, norm_weight, norm_bias, eps, w, bias, act, out),
                               x.device, x2.shape[0], N, K)
        if ok:
            return out.view(*x.shape[:-1], N)
    return linear(layer_norm(x, norm_weight, norm_bias, eps), weight, bias, act=act)


XADD = True   # route switch: False = `query + query_pos` as its own kernel / FFN output
# Rows from which `query + query_pos` is added inside the X-stationary kernel's operand load.  Until the encoder's two
# projections became one launch (encoder_projections) the 256-tile GEMM on a stored sum won below 400 000 rows (one
# 1920x1280 image: +0.09 ms per forward with the add folded in); with the one-launch form the fold wins at every size the
# kernel takes (one 1920x1280 image 13.14 -> 13.07 ms, one 1152x768 image 7.18 -> 7.15 ms), so the threshold is 0.
XADD_MIN_ROWS = 0


def linear_xadd_supported(x, x_add, weight):
    """True when (x + x_add) @ weight.T runs as ONE kernel (the add folded into the X-stationary GEMM's operand load)"""
    return (XADD and x.is_cuda and x_add is not None and x_add.shape == x.shape and x_add.dtype == x.dtype
            and weight.dtype == x.dtype and not torch.is_grad_enabled()
            and x.numel() // max(x.shape[-1], 1) >= XADD_MIN_ROWS
            and _cabi.linear_xadd_supported(x.numel() // max(x.shape[-1], 1), weight.shape[0], x.shape[-1], x.dtype))


def linear_xadd(x, x_add, weight, bias=None):
    """(x + x_add) @ weight.T + bias -- `query + query_pos` in front of the (offsets | logits) projection (reference
    multi_scale_deformable_attention.py:161-162, 177-179); the sum is rounded to the storage type first, exactly as
    the separate add.  Falls back to add + linear where the fused form does not apply."""
    _gpu(x, "linear_xadd")
    if linear_xadd_supported(x, x_add, weight):
        K, N = x.shape[-1], weight.shape[0]
        x2, a2 = x.reshape(-1, K), x_add.reshape(-1, K)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        a2 = a2 if a2.is_contiguous() else a2.contiguous()
        w = weight if weight.is_contiguous() else weight.contiguous()
        out = torch.empty((x2.shape[0], N), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            ok = _timed_linear(lambda: _cabi.linear_xadd(x2, a2, w, bias, out), x.device, x2.shape[0], N, K)
        if ok:
            return out.view(*x.shape[:-1], N)
    return linear(x + x_add, weight, bias)


# One 128-row block of the fused FFN kernel runs ~100 us (it walks the whole hidden dimension alone), and the chip
# holds 256 of them: below ~24k rows the grid is under one wave and the two plain GEMMs (which split N over blocks)
# finish sooner -- measured 98.6 us fused vs 27 us as two GEMMs at the decoder's 900 rows.
FFN_FUSED_MIN_ROWS = 24576


def ffn_fused_supported(x, w1, w2, act):
    return (x.is_cuda and x.numel() // max(x.shape[-1], 1) >= FFN_FUSED_MIN_ROWS
            and _cabi.ffn_fused_supported(x, w1, w2, act))


def derived(params, name, build):
    """A tensor derived from parameter tensors (fused / permuted / gathered weights), built once by `build()` and kept
    ON the first parameter object under attribute `name` -- so it dies with that parameter instead of sitting in a table
    keyed by an address the allocator can hand to a different tensor later.  Rebuilt when any source changed: object
    identity, in-place version counter, storage address (``param.data = ...``, ``.to()``), dtype or device."""
    first = params[0]
    key = tuple((id(p), p.data_ptr(), p._version, p.dtype, p.device) for p in params)
    hit = getattr(first, name, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        val = build()
    setattr(first, name, (key, val))
    return val


def _packed_w2(w2):
    """the kernel's pre-packed copy of a second-Linear weight.  The copy hangs on the weight tensor object itself
    (so it dies with it: a table keyed by id() / data_ptr() can hand a NEW tensor that reuses a freed tensor's address
    and id the old tensor's packed weights) and is rebuilt when the tensor is modified in place."""
    hit = getattr(w2, "_codetr_packed_w2", None)
    if hit is None or hit[0] != w2._version or hit[1].device != w2.device or hit[1].dtype != w2.dtype:
        with torch.no_grad(), torch.cuda.device(w2.device):
            hit = (w2._version, _cabi.ffn_pack_w2(w2.detach().contiguous()))
        w2._codetr_packed_w2 = hit
    return hit[1]


SWIN_MLP = True            # route switch (A/B): False = norm2 | fc1 + GELU | fc2 + identity as separate launches
SWIN_MLP_MIN_ROWS = 32768  # below this a stage's MLP is a few dozen tiles: the separate GEMMs fill the chip better


def swin_mlp_supported(x, ln_weight, w1, w2, act):
    """the fused Swin MLP (csrc/swin_mlp.hip) serves x [.., C] with C in {192, 384}, hidden = 4 C, GELU, 16-bit storage"""
    C = x.shape[-1]
    return (SWIN_MLP and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and act == "gelu" and C in (192, 384)
            and w1.shape == (4 * C, C) and w2.shape == (C, 4 * C) and ln_weight is not None
            and x.numel() // C >= SWIN_MLP_MIN_ROWS and w1.dtype == x.dtype and w2.dtype == x.dtype)


def swin_mlp(x, ln_weight, ln_bias, eps, w1, b1, w2, b2):
    """y = x + fc2(gelu(fc1(layer_norm(x)))): the second half of a SwinBlock in one launch (reference swin.py:331-352)"""
    _gpu(x, "swin_mlp")
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    out = torch.empty_like(x2)
    w1c = w1 if w1.is_contiguous() else w1.contiguous()
    with torch.cuda.device(x.device):
        w2p = _packed_w2(w2)
        _timed("swin_mlp", {"M": x2.shape[0], "C": C},
               lambda: _cabi.swin_mlp(x2, ln_weight, ln_bias, eps, w1c, b1, w2p, b2, out), x.device)
    return out.view(x.shape)


def ffn_fused(x, w1, b1, w2, b2, ln=None, pos=None, ln_in=None):
    """y = x + relu(x @ w1.T + b1) @ w2.T + b2 in one kernel (hidden activation stays on-chip); x [..., 256].
    w2 is the plain nn.Linear weight; its packed form is cached.
    ln = (weight, bias, eps): y = LayerNorm(y) in the same epilogue.  pos (same shape as x): also returns y + pos,
    i.e. the result is (y, y + pos).  ln_in = (weight, bias, eps): the input rows are LayerNorm'ed first (in
    registers; that norm's output is both the FFN input and the identity and is never written)."""
    _gpu(x, "ffn_fused")
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    out = torch.empty_like(x2)
    p2 = out2 = None
    if pos is not None:
        p2 = pos.reshape(-1, pos.shape[-1])
        if p2.shape != x2.shape or p2.dtype != x2.dtype:
            raise ValueError("pos must match x in shape and dtype")
        if not p2.is_contiguous():
            p2 = p2.contiguous()
        out2 = torch.empty_like(x2)
    if x2.shape[0] > 0:
        with torch.cuda.device(x.device):
            _timed("ffn_fused", {"M": x2.shape[0], "C": x2.shape[1], "hidden": w1.shape[0]},
                   lambda: _cabi.ffn_fused(x2, w1.contiguous(), b1, _packed_w2(w2), b2, out, ln, p2, out2, ln_in), x.device)
    if pos is not None:
        return out.view(x.shape), out2.view(x.shape)
    return out.view(x.shape)


FFN_OPROJ = True   # route switch: the encoder layer's attention output projection inside the fused FFN launch


def ffn_oproj_fused(attn, wo, bo, identity, w1, b1, w2, b2, ln, pos=None, ln_in=None):
    """The post-norm encoder layer from the attention output on, ONE launch (include/codetr_hip.h
    codetr_ffn_oproj_relu_ln2_*):  x1 = LN_in(identity + (attn @ wo.T + bo));  y = LN(x1 + relu(x1 @ w1.T + b1) @ w2.T + b2);
    with `pos` also y + pos (returns (y, y + pos)).  w1 / w2 are the plain nn.Linear weights (their kernel layouts are
    cached on the tensors)."""
    _gpu(attn, "ffn_oproj_fused")
    C = attn.shape[-1]
    a2, i2 = attn.reshape(-1, C), identity.reshape(-1, C)
    a2 = a2 if a2.is_contiguous() else a2.contiguous()
    i2 = i2 if i2.is_contiguous() else i2.contiguous()
    if i2.shape != a2.shape or i2.dtype != a2.dtype:
        raise ValueError("identity must match the attention output in shape and dtype")
    out = torch.empty_like(a2)
    p2 = out2 = None
    if pos is not None:
        p2 = pos.reshape(-1, C)
        if p2.shape != a2.shape or p2.dtype != a2.dtype:
            raise ValueError("pos must match x in shape and dtype")
        p2 = p2 if p2.is_contiguous() else p2.contiguous()
        out2 = torch.empty_like(a2)
    w1p = derived((w1,), "_codetr_w1_oproj", lambda: w1.detach()[:, torch.tensor(
        _cabi.ffn_oproj_w1_index(C), dtype=torch.long, device=w1.device)].contiguous())
    woc = wo if wo.is_contiguous() else wo.contiguous()
    if a2.shape[0] > 0:
        with torch.cuda.device(attn.device):
            _timed("ffn_fused", {"M": a2.shape[0], "C": C, "hidden": w1.shape[0], "oproj": True},
                   lambda: _cabi.ffn_oproj_fused(a2, woc, bo, i2, w1p, b1, _packed_w2(w2), b2, out, ln_in, ln, p2, out2),
                   attn.device)
    if pos is not None:
        return out.view(attn.shape), out2.view(attn.shape)
    return out.view(attn.shape)


def layer_norm(x, weight, bias, eps=1e-5):
    _gpu(x, "layer_norm")
    if _cabi.layernorm_supported(x, weight):
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        out = torch.empty_like(x2)
        if x2.shape[0] > 0:
            with torch.cuda.device(x.device):
                _cabi.layernorm(x2, weight, bias, eps, out)
        return out.view(x.shape)
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)  # fp32 parity runs


MERGE_LN = True   # route switch: False = separate patch-merge gather + LayerNorm


def patch_merge_layernorm_supported(x, C):
    return (x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and C % 8 == 0 and 4 * C <= 4096
            and MERGE_LN)


def patch_merge_layernorm(x, hw, weight_kkc, bias_kkc, eps=1e-5):
    """Swin PatchMerging's 2x2 gather + LayerNorm(4C) in one pass: x [B, H*W, C] tokens -> [B, H2*W2, 4C] with the 4C
    axis ordered (ky, kx, c) (weight / bias given in that order)."""
    _gpu(x, "patch_merge_layernorm")
    B, L, C = x.shape
    H, W = hw
    x4 = x.view(B, H, W, C)
    if not x4.is_contiguous():
        x4 = x4.contiguous()
    with torch.cuda.device(x.device):
        return _cabi.patch_merge_layernorm(x4, weight_kkc, bias_kkc, eps)


def group_norm(x, groups, weight, bias, eps=1e-5):
    _gpu(x, "group_norm")
    return F.group_norm(x, groups, weight, bias, eps)


def groupnorm_tokens_supported(x, groups):
    return x.is_cuda and _cabi.groupnorm_tokens_supported(x, groups)


def groupnorm_tokens_into(x, gamma, beta, groups, eps, dest, row_start):
    """GroupNorm of token-major x [B,HW,C] written into dest[:, row_start:row_start+HW, :] (dest [B,S,C] contiguous)."""
    _gpu(x, "groupnorm_tokens_into")
    B, HW, C = x.shape
    if not x.is_contiguous():
        x = x.contiguous()
    if not dest.is_contiguous() or dest.shape[0] != B or dest.shape[2] != C:
        raise AssertionError("destination must be a contiguous [B, S, C] tensor")
    with torch.cuda.device(x.device):
        _cabi.groupnorm_tokens(x, gamma, beta, groups, eps, dest[0, row_start:], dest.shape[1] * C)
    return dest


def query_sine_embed_supported(ref, valid_ratios, pos_feat):
    return (ref.is_cuda and ref.dtype in (torch.float16, torch.bfloat16) and valid_ratios.dtype == ref.dtype
            and ref.shape[-1] in (2, 4) and pos_feat % 8 == 0 and valid_ratios.shape[1] <= ref.shape[-1] * pos_feat // 8)


def query_sine_embed(ref, valid_ratios, pos_feat, temperature=10000.0):
    """Decoder layer head in one launch: (sigmoid(ref)[:, :, None] * valid_ratios (tiled to ref_dim)[:, None],
    gen_sineembed_for_position of its level-0 row) -- see include/codetr_hip.h.  When `valid_ratios` carries its fp32
    twin (``_codetr_f32``, hip_ops.valid_ratios), the returned ref_in carries ``_codetr_ref32``: the same reference points
    with sigmoid and scaling kept in fp32, which msda_fused then samples at."""
    _gpu(ref, "query_sine_embed")
    vr32 = getattr(valid_ratios, "_codetr_f32", None) if MSDA_FP32_REF else None
    with torch.cuda.device(ref.device):
        ref_in, embed, ref32 = _cabi.query_sine_embed(ref.contiguous(), valid_ratios.contiguous(), pos_feat, temperature,
                                                      valid_ratios32=vr32)
    if ref32 is not None:
        ref_in._codetr_ref32 = ref32
    return ref_in, embed


def encoder_geometry(valid_ratios, mask_flat, shapes):
    """Reference points, their per-level scaling, two-stage proposals (already masked) and the keep / drop state of
    every encoder token in one launch (csrc/encoder_geometry.hip); f16 valid_ratios [B,L,2], mask_flat [B,S] bool."""
    _gpu(mask_flat, "encoder_geometry")
    if valid_ratios.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("encoder_geometry is the 16-bit inference path; fp32 parity runs use the ATen formulation")
    with torch.cuda.device(mask_flat.device):
        return _cabi.encoder_geometry(valid_ratios.contiguous(), mask_flat.contiguous(),
                                      [tuple(int(v) for v in s) for s in shapes])


def row_max(x):
    """x.max(-1)[0] for a dense f16 tensor (NaN propagates)"""
    _gpu(x, "row_max")
    if x.dtype not in (torch.float16, torch.bfloat16) or not x.is_contiguous():
        return x.max(-1)[0]
    with torch.cuda.device(x.device):
        return _cabi.row_max(x.view(-1, x.shape[-1])).view(x.shape[:-1])


def preprocess_image(src_u8, resized_hw, pad_hw, mean, std, pad_value=(0, 0, 0), dtype=torch.float16):
    """uint8 HWC RGB image on the GPU -> (normalised [3, Hp, Wp], mask [Hp, Wp]): cv2-exact bilinear resize to
    `resized_hw`, right / bottom padding with `pad_value` to `pad_hw`, (x - mean) / std (csrc/prepost.hip)."""
    _gpu(src_u8, "preprocess_image")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 3 or src_u8.shape[2] != 3:
        raise ValueError("expected a uint8 [H, W, 3] image")
    with torch.cuda.device(src_u8.device):
        return _cabi.preprocess_u8(src_u8.contiguous(), resized_hw, pad_hw, mean, std, pad_value, dtype)


def batched_nms(boxes, scores, labels, iou_threshold):
    """torchvision.ops.batched_nms semantics (per-class greedy hard NMS): indices of the kept boxes in descending
    score order.  IoU arithmetic in fp32 on the given boxes."""
    _gpu(boxes, "batched_nms")
    if boxes.shape[0] == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores.float(), descending=True, stable=True)[1]
    with torch.cuda.device(boxes.device):
        keep = _cabi.batched_nms_sorted(boxes.float()[order].contiguous(), labels.to(torch.int64)[order].contiguous(),
                                        iou_threshold)
    return order[keep]


PREPROCESS_BATCH_MAX = _cabi.PREPROCESS_BATCH_MAX


def _preprocess_rows(name, launch, src_u8, rows, batch_hw, mean, std, pad_val, pad_value, dtype, with_mask):
    """the body of preprocess_batch and preprocess_views: one `launch` per PREPROCESS_BATCH_MAX rows into one batch"""
    _gpu(src_u8, name)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 1 or not src_u8.is_contiguous():
        raise ValueError("expected one contiguous flat uint8 buffer")
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"{name} writes f16, bf16 or f32, not {dtype}")
    N = len(rows)
    H, W = (int(v) for v in batch_hw)
    x = torch.empty((N, 3, H, W), dtype=dtype, device=src_u8.device)
    m = torch.empty((N, H, W), dtype=dtype, device=src_u8.device) if with_mask else None
    with torch.cuda.device(src_u8.device):
        for i in range(0, N, PREPROCESS_BATCH_MAX):
            j = min(N, i + PREPROCESS_BATCH_MAX)
            launch(src_u8, rows[i:j], (H, W), mean, std, pad_val, pad_value, x[i:j], m[i:j] if m is not None else None)
    return x, m


def preprocess_batch(src_u8, images, batch_hw, mean, std, pad_val=(0, 0, 0), pad_value=0.0, dtype=torch.float16,
                     with_mask=True):
    """Many uint8 HWC RGB images of different sizes, back to back in ONE flat device buffer -> the stacked
    (batch_inputs [N, 3, H, W], img_masks [N, H, W] or None), batch_hw = (H, W).  images: one row per image,
    (src_offset, H_src, W_src, H_resized, W_resized, H_pad, W_pad).  Per image preprocess_image's arithmetic into its
    (H_pad, W_pad) Pad region; beyond it `pad_value` as is and mask 1 (DetDataPreprocessor's divisor padding and
    stack_batch).  One launch per PREPROCESS_BATCH_MAX images (csrc/prepost.hip)."""
    return _preprocess_rows("preprocess_batch", _cabi.preprocess_batch_u8, src_u8, images, batch_hw, mean, std, pad_val,
                            pad_value, dtype, with_mask)


def preprocess_views(src_u8, rows8, batch_hw, mean, std, pad_val=(0, 0, 0), pad_value=0.0, dtype=torch.float16,
                     with_mask=True):
    """preprocess_batch for test-time augmentation's views: rows8 has one row per VIEW, (src_offset, H_src, W_src,
    H_resized, W_resized, H_pad, W_pad, flip).  flip = 1 writes the resized image mirrored left to right inside its
    resized width (mmdet flips after Resize and before any padding: the padding stays on the right, the mask does not
    change); rows may share a src_offset, so the views of an image read its one uploaded copy.  -> (batch_inputs
    [N, 3, H, W], img_masks [N, H, W] or None), N = len(rows8); one launch per PREPROCESS_BATCH_MAX rows."""
    if any(len(r) != 8 for r in rows8):
        raise ValueError("preprocess_views: eight values per row, the last one the flip (0 or 1)")
    return _preprocess_rows("preprocess_views", _cabi.preprocess_views_u8, src_u8, rows8, batch_hw, mean, std, pad_val,
                            pad_value, dtype, with_mask)


def preprocess_tiles(src_u8, rows11, batch_hw, mean, std, pad_val=(0, 0, 0), pad_value=0.0, dtype=torch.float16,
                     with_mask=True):
    """preprocess_batch for sliced inference's tiles: rows11 has one row per TILE, (src_offset, H_img, W_img, y0, x0,
    H_crop, W_crop, H_resized, W_resized, H_pad, W_pad).  A row is, bit for bit, what preprocess_batch writes for a
    contiguous copy of the H_crop x W_crop window at (y0, x0) of its image: the tile is resized as an image of its own
    and never reads a pixel outside the crop.  Rows may share a src_offset, so the tiles of an image read its one
    uploaded copy.  -> (batch_inputs [N, 3, H, W], img_masks [N, H, W] or None), N = len(rows11); one launch per
    PREPROCESS_BATCH_MAX rows."""
    if any(len(r) != 11 for r in rows11):
        raise ValueError("preprocess_tiles: eleven values per row (src_offset, H_img, W_img, y0, x0, H_crop, W_crop, "
                         "H_resized, W_resized, H_pad, W_pad)")
    return _preprocess_rows("preprocess_tiles", _cabi.preprocess_tiles_u8, src_u8, rows11, batch_hw, mean, std, pad_val,
                            pad_value, dtype, with_mask)


# postprocess_detections' result: boxes [N,Q,4] / scores [N,Q] (input dtype), labels [N,Q] int64, count [N] int32 --
# image i's detections are rows [:count[i]] -- all four views of the one byte buffer `packed`
Detections = collections.namedtuple("Detections", "boxes scores labels count packed")
# postprocess_detections_soft's and tta_merge's result: the fields of Detections + index [N,Q] int32, the input index
# of every output row -- five views of the one byte buffer `packed`
SoftDetections = collections.namedtuple("SoftDetections", "boxes scores labels count index packed")


def _detection_views(packed, N, Q, dtype, with_index):
    """the views of a packed result: labels, count, [index,] boxes, scores in this order"""
    es = torch.empty((), dtype=dtype).element_size()
    o1 = N * Q * 8
    o2 = o1 + N * 4
    o3 = o2 + (N * Q * 4 if with_index else 0)
    o4 = o3 + N * Q * 4 * es
    o5 = o4 + N * Q * es
    boxes, scores = packed[o3:o4].view(dtype).view(N, Q, 4), packed[o4:o5].view(dtype).view(N, Q)
    labels, count = packed[:o1].view(torch.int64).view(N, Q), packed[o1:o2].view(torch.int32)
    if not with_index:
        return Detections(boxes, scores, labels, count, packed)
    return SoftDetections(boxes, scores, labels, count, packed[o2:o3].view(torch.int32).view(N, Q), packed)


def _new_detections(N, Q, dtype, device, with_index, zeros):
    """the packed result over [N, Q] rows, for a launch to fill; `zeros`: nothing will be launched, every count is 0"""
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = N * Q * (12 if with_index else 8) + N * 4 + N * Q * 5 * es
    alloc = torch.zeros if zeros else torch.empty
    return _detection_views(alloc((nbytes,), dtype=torch.uint8, device=device), N, Q, dtype, with_index)


def _post_operands(name, boxes, scores, labels, divisors):
    """the operand checks of postprocess_detections and postprocess_detections_soft (`name`) -> N, Q"""
    dtype = scores.dtype
    if dtype not in (torch.float16, torch.bfloat16, torch.float32) or boxes.dtype != dtype or divisors.dtype != dtype:
        raise ValueError(f"{name}: boxes, scores and divisors in one dtype of f16 / bf16 / f32")
    shapes = f"{name}: boxes [N,Q,4], scores [N,Q], labels [N,Q], divisors [N,4]"
    if scores.dim() != 2:
        raise ValueError(shapes)
    N, Q = scores.shape
    if tuple(boxes.shape) != (N, Q, 4) or tuple(labels.shape) != (N, Q) or tuple(divisors.shape) != (N, 4):
        raise ValueError(shapes)
    return N, Q


def postprocess_detections(boxes, scores, labels, divisors, score_threshold=None, iou_threshold=None):
    """Inferencer.postprocess_predictions + run_inference's `boxes / scale_factor` for a whole batch in one launch
    (csrc/prepost.hip): boxes [N,Q,4], scores [N,Q], divisors [N,4] in one of f16 / bf16 / f32, labels [N,Q] int64,
    Q <= 1024.  score_threshold: keep `scores > score_threshold` (compared in the scores' dtype; None: no threshold);
    iou_threshold: per-class NMS in descending score order (None: none, index order kept).  -> Detections, compacted
    per image; `detections_to_host` fetches all of it in one copy."""
    _gpu(scores, "postprocess_detections")
    N, Q = _post_operands("postprocess_detections", boxes, scores, labels, divisors)
    nothing = N == 0 or Q == 0
    out = _new_detections(N, Q, scores.dtype, scores.device, False, nothing)
    if nothing:
        return out
    with torch.cuda.device(scores.device):
        _cabi.postprocess_detections(boxes.contiguous(), scores.contiguous(), labels.to(torch.int64).contiguous(),
                                     divisors.contiguous(), score_threshold, iou_threshold, out.boxes, out.scores,
                                     out.labels, out.count)
    return out


def detections_to_host(dets):
    """postprocess_detections' (or postprocess_detections_soft's, `index` included) result on the host: one
    device-to-host copy of the packed buffer"""
    N, Q = dets.scores.shape
    if isinstance(dets, WbfDetections):
        return _wbf_views(dets.packed.cpu(), N, Q, dets.scores.dtype)
    return _detection_views(dets.packed.cpu(), N, Q, dets.scores.dtype, isinstance(dets, SoftDetections))


def _soft_method(method):
    if method == "gaussian":
        raise NotImplementedError("soft-NMS method 'gaussian' is not provided (exp() cannot be held bit-exact against "
                                  "the CPU reference and no shipped config uses it): 'linear' or 'naive'")
    if method not in _cabi.SOFTNMS_METHODS:
        raise ValueError(f"soft-NMS method must be 'linear' or 'naive', got {method!r}")
    return _cabi.SOFTNMS_METHODS[method]


def postprocess_detections_soft(boxes, scores, labels, divisors, score_threshold=None, iou_threshold=0.3,
                                method="linear", min_score=1e-3, max_per_img=None):
    """The post-processing the model configs specify (test_cfg[0]: nms type 'soft_nms', max_per_img) + run_inference's
    `boxes / scale_factor` for a whole batch in one launch (csrc/prepost.hip; semantics: include/codetr_hip.h): mmcv's
    soft-NMS per class -- overlapping boxes are not removed but their scores decayed by 1 - IoU (`linear`) or set to 0
    (`naive`) when IoU >= iou_threshold, a box leaves once its score is < min_score --, the detections sorted by decayed
    score, the first max_per_img kept (None: all).  Operands as postprocess_detections; the defaults are mmcv's.
    -> SoftDetections: scores are the decayed ones, `index` the query index of every row."""
    _gpu(scores, "postprocess_detections_soft")
    m = _soft_method(method)
    N, Q = _post_operands("postprocess_detections_soft", boxes, scores, labels, divisors)
    nothing = N == 0 or Q == 0
    out = _new_detections(N, Q, scores.dtype, scores.device, True, nothing)
    if nothing:
        return out
    with torch.cuda.device(scores.device):
        _cabi.postprocess_softnms(boxes.contiguous(), scores.contiguous(), labels.to(torch.int64).contiguous(),
                                  divisors.contiguous(), score_threshold, m, iou_threshold, min_score,
                                  0 if max_per_img is None else int(max_per_img), out.boxes, out.scores, out.labels,
                                  out.index, out.count)
    return out


def soft_nms(boxes, scores, labels, iou_threshold, method="linear", min_score=1e-3):
    """mmcv batched_nms(..., nms_cfg=dict(type='soft_nms')) semantics for one image's detections (boxes [n,4],
    scores [n], labels [n]; n <= 1024), the counterpart of `batched_nms`: -> (new_scores, keep), the decayed scores of
    the kept boxes in descending order (dtype of `scores`) and their indices.  The N = 1 launch of
    postprocess_detections_soft with unit divisors."""
    _gpu(boxes, "soft_nms")
    _soft_method(method)
    n = boxes.shape[0]
    if n == 0:
        return scores.new_empty((0,)), torch.empty((0,), dtype=torch.int64, device=boxes.device)
    if n > _cabi.POSTPROCESS_MAX_Q:
        raise ValueError(f"soft_nms: at most {_cabi.POSTPROCESS_MAX_Q} boxes per call, got {n}")
    dtype = scores.dtype if scores.dtype in (torch.float16, torch.bfloat16, torch.float32) else torch.float32
    dets = postprocess_detections_soft(boxes.to(dtype)[None], scores.to(dtype)[None], labels[None],
                                       torch.ones((1, 4), dtype=dtype, device=boxes.device), None, iou_threshold, method,
                                       min_score, None)
    c = int(dets.count[0])
    return dets.scores[0, :c].to(scores.dtype), dets.index[0, :c].to(torch.int64)


TTA_MAX_VIEWS = _cabi.TTA_MAX_VIEWS
TTA_MAX_CANDIDATES = _cabi.TTA_MAX_CANDIDATES


def _tta_mode(nms):
    """tta_cfg.nms -> (mode of codetr_tta_merge_*, iou_threshold, min_score); mmcv's defaults where a key is absent"""
    kind = nms.get("type", "nms")
    if kind == "nms":
        return _cabi.TTA_NMS_MODES["nms"], float(nms.get("iou_threshold", 0.5)), 0.0
    if kind != "soft_nms":
        raise NotImplementedError(f"tta nms type {kind!r}: 'nms' and 'soft_nms' are built")
    method = nms.get("method", "linear")
    _soft_method(method)   # 'gaussian' raises NotImplementedError, an unknown name ValueError
    return _cabi.TTA_NMS_MODES[method], float(nms.get("iou_threshold", 0.3)), float(nms.get("min_score", 1e-3))


def _merge_operands(name, view_dets, flips, widths):
    """the operand checks of tta_merge and wbf_merge (`name`) -> (dtype, device, N, V, Q, boxes, scores, labels, count,
    flips, widths): the entries concatenated in order, `widths` a tensor"""
    if not view_dets:
        raise ValueError(f"{name}: no views")
    scores0 = view_dets[0].scores
    _gpu(scores0, name)
    dtype, dev, Q = scores0.dtype, scores0.device, scores0.shape[-1]
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"{name}: detections in f16, bf16 or f32")
    if not torch.is_tensor(widths):
        widths = torch.tensor([float(w) for w in widths], dtype=torch.float32)
    N = widths.numel()
    if N == 0 or any(d.scores.dim() != 2 or d.scores.shape[0] % N or d.scores.shape[1] != Q or d.scores.dtype != dtype
                     for d in view_dets):
        raise ValueError(f"{name}: every entry [views * N, Q] detections of one dtype, N = len(widths) > 0")
    V = sum(d.scores.shape[0] for d in view_dets) // N
    flips = [bool(f) for f in flips]
    if len(flips) != V:
        raise ValueError(f"{name}: {V} views but {len(flips)} flip flags")
    if V > TTA_MAX_VIEWS or V * Q > TTA_MAX_CANDIDATES:
        raise ValueError(f"{name}: at most {TTA_MAX_VIEWS} views and {TTA_MAX_CANDIDATES} candidates per image, "
                         f"got {V} views of {Q}")
    one = len(view_dets) == 1
    boxes = (view_dets[0].boxes if one else torch.cat([d.boxes for d in view_dets])).contiguous()
    scores = (view_dets[0].scores if one else torch.cat([d.scores for d in view_dets])).contiguous()
    labels = (view_dets[0].labels if one else torch.cat([d.labels for d in view_dets])).contiguous()
    count = (view_dets[0].count if one else torch.cat([d.count for d in view_dets])).contiguous()
    return dtype, dev, N, V, Q, boxes, scores, labels, count, flips, widths


def tta_merge(view_dets, flips, widths, nms=None, max_per_img=None):
    """mmdet DetTTAModel._merge_single_sample for a batch of N images in one launch (csrc/prepost.hip; semantics:
    include/codetr_hip.h): the views' detections un-flipped, concatenated, batched_nms(nms), the best max_per_img kept.
      view_dets    the per-view results of postprocess_detections / postprocess_detections_soft, boxes already in
                   original-image coordinates.  Each entry holds one or more views of all N images, view-major (its
                   leading dimension is a multiple of N); the entries are concatenated in order, so view v is row block v
      flips        one bool per view: the view was flipped horizontally
      widths       [N] original image widths (a tensor on the device, or numbers)
      nms          dict(type='nms' | 'soft_nms', iou_threshold, [method 'linear' | 'naive', min_score]); None: hard, 0.5
      max_per_img  None: all
    -> SoftDetections over [N, K] rows (K = max_per_img, or V * Q): `index` is c = v * Q + j of every row, scores are
    the decayed ones in the soft modes; `detections_to_host` fetches all of it in one copy."""
    mode, iou, min_score = _tta_mode(dict(nms) if nms is not None else {})
    dtype, dev, N, V, Q, boxes, scores, labels, count, flips, widths = _merge_operands("tta_merge", view_dets, flips, widths)
    keep = 0 if max_per_img is None else int(max_per_img)
    K = keep if keep > 0 else V * Q
    out = _new_detections(N, K, dtype, dev, True, Q == 0)
    if Q == 0:
        return out
    with torch.cuda.device(dev):
        _cabi.tta_merge(boxes.view(V, N, Q, 4), scores.view(V, N, Q), labels.view(V, N, Q), count.view(V, N),
                        sum(1 << v for v, f in enumerate(flips) if f), widths.to(dev, torch.float32).contiguous(), mode,
                        iou, min_score, keep, out.boxes, out.scores, out.labels, out.index, out.count)
    return out


# wbf_merge's result: the fields of SoftDetections + votes [N,K] int32, the number of candidates fused into every row --
# six views of the one byte buffer `packed` (labels, count, index, votes, boxes, scores in this order)
WbfDetections = collections.namedtuple("WbfDetections", "boxes scores labels count index votes packed")
WBF_MAX_CANDIDATES = _wbf.MAX_CANDIDATES
WBF = dict(iou_threshold=0.55, skip_box_thr=0.0, conf_type="avg", weights=None)   # ensemble_boxes' defaults


def _wbf_views(packed, N, K, dtype):
    es = torch.empty((), dtype=dtype).element_size()
    o1 = N * K * 8
    o2 = o1 + N * 4
    o3 = o2 + N * K * 4
    o4 = o3 + N * K * 4
    o5 = o4 + N * K * 4 * es
    o6 = o5 + N * K * es
    return WbfDetections(packed[o4:o5].view(dtype).view(N, K, 4), packed[o5:o6].view(dtype).view(N, K),
                         packed[:o1].view(torch.int64).view(N, K), packed[o1:o2].view(torch.int32),
                         packed[o2:o3].view(torch.int32).view(N, K), packed[o3:o4].view(torch.int32).view(N, K), packed)


def wbf_settings(d=None):
    """the `wbf` dict of a weighted boxes fusion, validated and completed from WBF -> dict(iou_threshold, skip_box_thr,
    conf_type 'avg' | 'max', weights None or a list of positive floats)"""
    if d is not None and not isinstance(d, dict):
        raise ValueError(f"wbf must be None or a dict with keys of {sorted(WBF)}")
    out = dict(WBF)
    unknown = set(d or {}) - set(out)
    if unknown:
        raise ValueError(f"wbf: unknown key(s) {sorted(unknown)}; known: {sorted(out)}")
    out.update(d or {})
    if out["conf_type"] in ("box_and_model_avg", "absent_model_aware_avg"):
        raise NotImplementedError(f"wbf conf_type {out['conf_type']!r} is not built: 'avg' or 'max'")
    if out["conf_type"] not in _wbf.CONF_TYPES:
        raise ValueError(f"wbf conf_type must be 'avg' or 'max', got {out['conf_type']!r}")
    for key in ("iou_threshold", "skip_box_thr"):
        out[key] = float(out[key])
        if not math.isfinite(out[key]):
            raise ValueError(f"wbf {key} must be finite")
    if out["weights"] is not None:
        out["weights"] = [float(w) for w in out["weights"]]
        if not out["weights"] or any(not math.isfinite(w) or w <= 0 for w in out["weights"]):
            raise ValueError("wbf weights: None or a non-empty list of finite positive numbers")
    return out


def wbf_merge(view_dets, flips, widths, wbf=None, max_per_img=None):
    """Weighted boxes fusion of the views' detections for a batch of N images in one launch (csrc/prepost.hip; the rule:
    include/codetr_wbf.h): un-flipped, clustered per label in descending confidence, every cluster emitted as its
    confidence-weighted mean box with a score that says how many views agreed; the best max_per_img kept.
      view_dets, flips, widths, max_per_img   as tta_merge
      wbf          dict(iou_threshold, skip_box_thr, conf_type 'avg' | 'max', weights: one per view); None: WBF
    -> WbfDetections over [N, K] rows (K = max_per_img, or V * Q): `index` is the c = v * Q + j of every row's founder,
    `votes` its number of members; `detections_to_host` fetches all of it in one copy."""
    w = wbf_settings(wbf)
    dtype, dev, N, V, Q, boxes, scores, labels, count, flips, widths = _merge_operands("wbf_merge", view_dets, flips, widths)
    if V * Q > WBF_MAX_CANDIDATES:
        raise ValueError(f"wbf_merge: at most {WBF_MAX_CANDIDATES} candidates per image, got {V} views of {Q}")
    if w["weights"] is not None and len(w["weights"]) != V:
        raise ValueError(f"wbf_merge: {V} views but {len(w['weights'])} weights")
    keep = 0 if max_per_img is None else int(max_per_img)
    K = keep if keep > 0 else V * Q
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = N * K * 16 + N * 4 + N * K * 5 * es
    out = _wbf_views((torch.zeros if Q == 0 else torch.empty)((nbytes,), dtype=torch.uint8, device=dev), N, K, dtype)
    if Q == 0:
        return out
    with torch.cuda.device(dev):
        _wbf.wbf_merge(boxes.view(V, N, Q, 4), scores.view(V, N, Q), labels.view(V, N, Q), count.view(V, N),
                       sum(1 << v for v, f in enumerate(flips) if f), widths.to(dev, torch.float32).contiguous(),
                       w["weights"], _wbf.CONF_TYPES[w["conf_type"]], w["iou_threshold"], w["skip_box_thr"], keep,
                       out.boxes, out.scores, out.labels, out.index, out.count, out.votes)
    return out


def weighted_boxes_fusion(boxes_list, scores_list, labels_list, weights=None, iou_thr=0.55, skip_box_thr=0.0,
                          conf_type="avg"):
    """`ensemble_boxes.weighted_boxes_fusion`'s call shape for one image, the counterpart of `soft_nms`: one entry per
    model (or view) in each list -- boxes [n_i, 4], scores [n_i], labels [n_i], tensors on the GPU or array-likes; pixel
    or normalised coordinates -- `weights` one per entry.  -> (boxes [E, 4], scores [E], labels [E] int64) in descending
    score order, fp32 on the GPU.  The ragged lists are padded into the [V, 1, Q] operands of one wbf_merge launch; the
    rule and its deviations from the package are include/codetr_wbf.h's (parity is unpinned)."""
    V = len(scores_list)
    if V == 0 or len(boxes_list) != V or len(labels_list) != V:
        raise ValueError("weighted_boxes_fusion: boxes_list, scores_list and labels_list of one length > 0")
    dev = next((t.device for t in scores_list if torch.is_tensor(t) and t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    sc = [torch.as_tensor(s, dtype=torch.float32).reshape(-1).to(dev) for s in scores_list]
    bx = [torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4).to(dev) for b in boxes_list]
    lb = [torch.as_tensor(l).reshape(-1).to(dev, torch.int64) for l in labels_list]
    if any(b.shape[0] != s.shape[0] or l.shape[0] != s.shape[0] for b, s, l in zip(bx, sc, lb)):
        raise ValueError("weighted_boxes_fusion: every entry n boxes [n, 4], n scores and n labels")
    Q = max(s.shape[0] for s in sc)
    if Q == 0:
        return (torch.zeros((0, 4), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.float32, device=dev),
                torch.zeros((0,), dtype=torch.int64, device=dev))
    boxes = torch.zeros((V, Q, 4), dtype=torch.float32, device=dev)
    scores = torch.zeros((V, Q), dtype=torch.float32, device=dev)
    labels = torch.zeros((V, Q), dtype=torch.int64, device=dev)
    for v in range(V):
        n = sc[v].shape[0]
        boxes[v, :n], scores[v, :n], labels[v, :n] = bx[v], sc[v], lb[v]
    count = torch.tensor([s.shape[0] for s in sc], dtype=torch.int32, device=dev)
    dets = wbf_merge([Detections(boxes, scores, labels, count, None)], [False] * V, [0.0],
                     dict(iou_threshold=iou_thr, skip_box_thr=skip_box_thr, conf_type=conf_type,
                          weights=None if weights is None else list(weights)))
    c = int(dets.count[0])
    return dets.boxes[0, :c], dets.scores[0, :c], dets.labels[0, :c]


SLICE_MAX_VIEWS = _cabi.SLICE_MAX_VIEWS
SLICE_MERGE = dict(type="nmm", metric="ios", threshold=0.5, class_agnostic=False)   # SAHI's defaults


def slice_merge_settings(merge=None):
    """the `merge` dict of sliced inference, validated and completed from SLICE_MERGE -> dict(type 'nmm' | 'nms',
    metric 'ios' | 'iou', threshold, class_agnostic)"""
    out = dict(SLICE_MERGE)
    unknown = set(merge or {}) - set(out)
    if unknown:
        raise ValueError(f"slice merge: unknown key(s) {sorted(unknown)}; known: {sorted(out)}")
    out.update(merge or {})
    if out["type"] not in _cabi.SLICE_MODES:
        raise ValueError(f"slice merge type must be 'nmm' or 'nms', got {out['type']!r}")
    if out["metric"] not in _cabi.SLICE_METRICS:
        raise ValueError(f"slice merge metric must be 'ios' or 'iou', got {out['metric']!r}")
    out["threshold"] = float(out["threshold"])
    if not math.isfinite(out["threshold"]):
        raise ValueError("slice merge threshold must be finite")
    out["class_agnostic"] = bool(out["class_agnostic"])
    return out


def slice_merge(dets, rows, origins, sizes, merge=None, max_per_img=None):
    """The fusion of sliced inference's per-tile detections for N images in one launch (csrc/prepost.hip; semantics:
    include/codetr_hip.h): every row's boxes shifted by its tile's origin and clipped to the image, then per label (or
    over all labels) greedy NMS, or greedy non-maximum merging in which a pick absorbs what it retires into the box
    around them, under IoU or IoS (intersection over the smaller area); the best max_per_img kept.
      dets         the results of postprocess_detections / postprocess_detections_soft over R rows (one entry, or a
                   list concatenated in order), boxes in each crop's own pixel coordinates
      rows         [N, V] int32: the row of image n's v-th view; a value outside [0, R) is an absent view
      origins      [R, 2] fp32 (x0, y0) of every row's crop;  sizes  [N, 2] fp32 (W, H) of the original images
                   (tensors on the device, or nested lists)
      merge        dict(type 'nmm' | 'nms', metric 'ios' | 'iou', threshold, class_agnostic); None: SLICE_MERGE
      max_per_img  None: all
    -> SoftDetections over [N, K] rows (K = max_per_img, or V * Q): `index` is c = v * Q + j of every row (of the pick, in
    'nmm'); `detections_to_host` fetches all of it in one copy."""
    m = slice_merge_settings(merge)
    dets = list(dets) if isinstance(dets, (list, tuple)) and not hasattr(dets, "scores") else [dets]
    if not dets:
        raise ValueError("slice_merge: no detections")
    scores0 = dets[0].scores
    _gpu(scores0, "slice_merge")
    dtype, dev, Q = scores0.dtype, scores0.device, scores0.shape[-1]
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError("slice_merge: detections in f16, bf16 or f32")
    if any(d.scores.dim() != 2 or d.scores.shape[1] != Q or d.scores.dtype != dtype for d in dets):
        raise ValueError("slice_merge: every entry [rows, Q] detections of one dtype")
    R = sum(d.scores.shape[0] for d in dets)
    rows = torch.as_tensor(rows, dtype=torch.int32)
    origins = torch.as_tensor(origins, dtype=torch.float32)
    sizes = torch.as_tensor(sizes, dtype=torch.float32)
    if rows.dim() != 2 or rows.numel() == 0 or tuple(origins.shape) != (R, 2) or tuple(sizes.shape) != (rows.shape[0], 2):
        raise ValueError("slice_merge: rows [N, V], origins [R, 2], sizes [N, 2] with N, V > 0")
    N, V = rows.shape
    if V > SLICE_MAX_VIEWS or V * Q > TTA_MAX_CANDIDATES:
        raise ValueError(f"slice_merge: at most {SLICE_MAX_VIEWS} views and {TTA_MAX_CANDIDATES} candidates per image, "
                         f"got {V} views of {Q}")
    one = len(dets) == 1
    boxes = (dets[0].boxes if one else torch.cat([d.boxes for d in dets])).contiguous()
    scores = (dets[0].scores if one else torch.cat([d.scores for d in dets])).contiguous()
    labels = (dets[0].labels if one else torch.cat([d.labels for d in dets])).contiguous()
    count = (dets[0].count if one else torch.cat([d.count for d in dets])).contiguous()
    keep = 0 if max_per_img is None else int(max_per_img)
    K = keep if keep > 0 else V * Q
    out = _new_detections(N, K, dtype, dev, True, Q == 0 or R == 0)
    if Q == 0 or R == 0:
        return out
    with torch.cuda.device(dev):
        _cabi.slice_merge(boxes, scores, labels, count, rows.to(dev).contiguous(), origins.to(dev).contiguous(),
                          sizes.to(dev).contiguous(), _cabi.SLICE_METRICS[m["metric"]], _cabi.SLICE_MODES[m["type"]],
                          m["threshold"], m["class_agnostic"], keep, out.boxes, out.scores, out.labels, out.index,
                          out.count)
    return out


DRAW_MAX_Q = _cabi.DRAW_MAX_Q
DRAW_MAX_SIDE = _cabi.DRAW_MAX_SIDE
DRAW_NAME_ROW = 24    # bytes per row of the names table: the length, then up to 23 characters
# the defaults of mmdet's DetLocalVisualizer (line_width, alpha, text_color) and of the Inferencer's pred_score_thr
DRAW_STYLE = dict(line_width=3, alpha=0.8, score_thr=0.3, text_color=(200, 200, 200), font_scale=1, draw_labels=True)


def draw_style(style=None):
    """the style of draw_detections, validated: the keys of DRAW_STYLE (missing ones take its values) -> a new dict.
    ValueError for an unknown key, line_width outside 1..15, alpha outside [0, 1], font_scale outside 1..4, a
    text_color that is not three values in 0..255, a score_thr that is not a number."""
    st = dict(DRAW_STYLE)
    style = dict(style or {})
    unknown = set(style) - set(st)
    if unknown:
        raise ValueError(f"draw style: unknown key(s) {sorted(unknown)}; known: {sorted(st)}")
    st.update(style)

    def whole(key, lo, hi):
        v = st[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or not lo <= v <= hi:
            raise ValueError(f"draw style: {key} must be an integer in {lo}..{hi}, got {v!r}")
        return int(v)

    st["line_width"] = whole("line_width", 1, 15)
    st["font_scale"] = whole("font_scale", 1, 4)
    if isinstance(st["alpha"], bool) or not isinstance(st["alpha"], (int, float)) or not 0.0 <= st["alpha"] <= 1.0:
        raise ValueError(f"draw style: alpha must be in [0, 1], got {st['alpha']!r}")
    thr = st["score_thr"]
    if isinstance(thr, bool) or not isinstance(thr, (int, float)) or thr != thr:
        raise ValueError(f"draw style: score_thr must be a number, got {thr!r}")
    tc = st["text_color"]
    if not isinstance(tc, (tuple, list)) or len(tc) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in tc):
        raise ValueError(f"draw style: text_color must be three values in 0..255, got {tc!r}")
    st["alpha"], st["score_thr"], st["text_color"] = float(st["alpha"]), float(thr), tuple(int(v) for v in tc)
    st["draw_labels"] = bool(st["draw_labels"])
    return st


def draw_names_table(classes):
    """class names -> the [C, 24] uint8 table draw_detections reads (a CPU tensor): byte 0 of a row is the length, the
    name truncated to 23 characters; a character outside ASCII 32..126 becomes '?'"""
    rows = []
    for name in classes:
        text = "".join(ch if 32 <= ord(ch) <= 126 else "?" for ch in str(name))[:DRAW_NAME_ROW - 1]
        rows.append(bytes([len(text)]) + text.encode("ascii") + bytes(DRAW_NAME_ROW - 1 - len(text)))
    return torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).view(len(rows), DRAW_NAME_ROW)


def draw_detections(buf_u8, rows, dets, names, palette, style=None):
    """The Inferencer's visualisation in one launch per PREPROCESS_BATCH_MAX images (csrc/draw.hip; the rendering is
    stated in include/codetr_hip.h): per detection with a score above style['score_thr'] a box outline in its class
    colour and, after all outlines, "<name>: <percent>" on a darkened patch at the box's top-left corner.  In place.
      buf_u8    one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows      (offset, H, W) per image
      dets      Detections / SoftDetections over [N, Q] rows, N = len(rows), Q <= 4096, boxes in image coordinates
      names     [C, 24] uint8 on the device (draw_names_table); palette [C, 3] uint8 on the device
      style     the keys of DRAW_STYLE
    -> buf_u8.  ValueError for Q > 4096, a bad style value, a wrong dtype or shape, CPU tensors.  Nothing is launched
    when N == 0 or Q == 0."""
    st = draw_style(style)
    tensors = dict(buf=buf_u8, names=names, palette=palette, boxes=dets.boxes, scores=dets.scores, labels=dets.labels,
                   count=dets.count)
    for key, t in tensors.items():
        if not torch.is_tensor(t) or not t.is_cuda or t.device != buf_u8.device:
            raise ValueError(f"draw_detections: {key} must be a tensor on the image buffer's GPU")
    if buf_u8.dtype != torch.uint8 or buf_u8.dim() != 1 or not buf_u8.is_contiguous():
        raise ValueError("draw_detections: expected one contiguous flat uint8 buffer")
    C = palette.shape[0] if palette.dim() == 2 else 0
    if names.dtype != torch.uint8 or palette.dtype != torch.uint8 or C == 0 or tuple(palette.shape) != (C, 3) or \
            tuple(names.shape) != (C, DRAW_NAME_ROW):
        raise ValueError("draw_detections: names [C, 24] and palette [C, 3] in uint8, C > 0")
    dtype = dets.scores.dtype
    if dtype not in (torch.float16, torch.bfloat16, torch.float32) or dets.boxes.dtype != dtype or \
            dets.labels.dtype != torch.int64 or dets.count.dtype != torch.int32:
        raise ValueError("draw_detections: boxes and scores in one dtype of f16 / bf16 / f32, labels int64, count int32")
    rows = [tuple(int(v) for v in r) for r in rows]
    N = len(rows)
    if dets.scores.dim() != 2 or dets.scores.shape[0] != N or tuple(dets.boxes.shape) != tuple(dets.scores.shape) + (4,) \
            or dets.labels.shape != dets.scores.shape or tuple(dets.count.shape) != (N,):
        raise ValueError("draw_detections: boxes [N,Q,4], scores [N,Q], labels [N,Q], count [N], N = len(rows)")
    Q = dets.scores.shape[1]
    if Q > DRAW_MAX_Q:
        raise ValueError(f"draw_detections: at most {DRAW_MAX_Q} detection rows per image, got {Q}")
    for off, H, W in rows:
        if not (1 <= H <= DRAW_MAX_SIDE and 1 <= W <= DRAW_MAX_SIDE) or off < 0 or off + H * W * 3 > buf_u8.numel():
            raise ValueError(f"draw_detections: image (offset {off}, {H}x{W}) outside the buffer or larger than "
                             f"{DRAW_MAX_SIDE} a side")
    if N == 0 or Q == 0:
        return buf_u8
    boxes, scores, labels, count = (t.contiguous() for t in (dets.boxes, dets.scores, dets.labels, dets.count))
    tc = st["text_color"]
    with torch.cuda.device(buf_u8.device):
        for i in range(0, N, PREPROCESS_BATCH_MAX):
            j = min(N, i + PREPROCESS_BATCH_MAX)
            _cabi.draw_detections(buf_u8, rows[i:j], boxes[i:j], scores[i:j], labels[i:j], count[i:j],
                                  palette.contiguous(), names.contiguous(), st["line_width"], st["alpha"], st["score_thr"],
                                  (tc[0] << 16) | (tc[1] << 8) | tc[2], st["font_scale"], st["draw_labels"])
    return buf_u8


# redaction of detected regions (include/codetr_redact.h states the rule and its limits).  "blur" is the library's own: a
# box filter over fixed cells and a tent reconstruction; parity with OpenCV's blur is unpinned (cv2 is not installed here)
REDACT = dict(mode="pixelate", score_thr=0.3, expand=0.1, shape="box", cell=16, fill=(0, 0, 0))
REDACT_MODES = tuple(_redact.MODES)
REDACT_SHAPES = tuple(_redact.SHAPES)
REDACT_CELLS = _redact.CELLS
_redact_work = {}   # device -> the "blur" workspace on it (uint8), grown when a call needs more


def redact_style(settings=None):
    """the settings of redact_detections, validated and completed from REDACT -> a new dict.  ValueError, naming the key,
    for an unknown key, a mode outside REDACT_MODES, a shape outside REDACT_SHAPES, a cell outside REDACT_CELLS, an expand
    outside [0, 1], a score_thr that is not a number, a fill that is not three whole values in 0..255."""
    st = dict(REDACT)
    settings = dict(settings or {})
    unknown = set(settings) - set(st)
    if unknown:
        raise ValueError(f"redact: unknown key(s) {sorted(unknown)}; known: {sorted(st)}")
    st.update(settings)

    def number(key):
        v = st[key]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
            raise ValueError(f"redact: {key} must be a number, got {v!r}")
        return float(v)

    if not isinstance(st["mode"], str) or st["mode"] not in REDACT_MODES:
        raise ValueError(f"redact: mode must be one of {list(REDACT_MODES)}, got {st['mode']!r}")
    if not isinstance(st["shape"], str) or st["shape"] not in REDACT_SHAPES:
        raise ValueError(f"redact: shape must be one of {list(REDACT_SHAPES)}, got {st['shape']!r}")
    cell = st["cell"]
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or int(cell) not in REDACT_CELLS:
        raise ValueError(f"redact: cell must be one of {list(REDACT_CELLS)}, got {cell!r}")
    st["cell"] = int(cell)
    st["score_thr"] = number("score_thr")
    st["expand"] = number("expand")
    if not 0.0 <= st["expand"] <= 1.0:
        raise ValueError(f"redact: expand must be in [0, 1], got {st['expand']!r}")
    fill = st["fill"]
    if not isinstance(fill, (tuple, list)) or len(fill) != 3 or any(
            isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or
            not 0 <= v <= 255 for v in fill):
        raise ValueError(f"redact: fill must be three whole values in 0..255, got {fill!r}")
    st["fill"] = tuple(int(v) for v in fill)
    return st


def redact_detections(buf_u8, rows, dets, settings=None, select=None):
    """Redaction of the detected regions in one launch per PREPROCESS_BATCH_MAX images ("blur": two) and without a
    synchronisation (csrc/redact.hip; include/codetr_redact.h states the rule): the pixels under every detection with a
    score above settings['score_thr'] and a selected label -- its box grown by settings['expand'], or the ellipse inside
    it -- become the mean of their cell ("pixelate"), the tent interpolation of the cell means ("blur") or
    settings['fill'].  In place; an unmasked pixel is never written.
      buf_u8    one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows      (offset, H, W) per image
      dets      Detections / SoftDetections over [N, Q] rows, N = len(rows), Q <= 4096, boxes in image coordinates
      settings  the keys of REDACT
      select    [C] uint8 on the device, 1 = redact this label (any other label is left); None = every label
    -> buf_u8.  ValueError for Q > 4096, a bad setting, a wrong dtype or shape, CPU tensors.  Nothing is launched when
    N == 0 or Q == 0.  "blur" keeps one workspace per device and grows it."""
    st = redact_style(settings)
    tensors = dict(buf=buf_u8, boxes=dets.boxes, scores=dets.scores, labels=dets.labels, count=dets.count)
    if select is not None:
        tensors["select"] = select
    for key, t in tensors.items():
        if not torch.is_tensor(t) or not t.is_cuda or t.device != buf_u8.device:
            raise ValueError(f"redact_detections: {key} must be a tensor on the image buffer's GPU")
    if buf_u8.dtype != torch.uint8 or buf_u8.dim() != 1 or not buf_u8.is_contiguous():
        raise ValueError("redact_detections: expected one contiguous flat uint8 buffer")
    if select is not None and (select.dtype != torch.uint8 or select.dim() != 1 or select.numel() == 0):
        raise ValueError("redact_detections: select must be a [C] uint8 table, C > 0")
    dtype = dets.scores.dtype
    if dtype not in (torch.float16, torch.bfloat16, torch.float32) or dets.boxes.dtype != dtype or \
            dets.labels.dtype != torch.int64 or dets.count.dtype != torch.int32:
        raise ValueError("redact_detections: boxes and scores in one dtype of f16 / bf16 / f32, labels int64, count int32")
    rows = [tuple(int(v) for v in r) for r in rows]
    N = len(rows)
    if dets.scores.dim() != 2 or dets.scores.shape[0] != N or tuple(dets.boxes.shape) != tuple(dets.scores.shape) + (4,) \
            or dets.labels.shape != dets.scores.shape or tuple(dets.count.shape) != (N,):
        raise ValueError("redact_detections: boxes [N,Q,4], scores [N,Q], labels [N,Q], count [N], N = len(rows)")
    Q = dets.scores.shape[1]
    if Q > DRAW_MAX_Q:
        raise ValueError(f"redact_detections: at most {DRAW_MAX_Q} detection rows per image, got {Q}")
    for off, H, W in rows:
        if not (1 <= H <= DRAW_MAX_SIDE and 1 <= W <= DRAW_MAX_SIDE) or off < 0 or off + H * W * 3 > buf_u8.numel():
            raise ValueError(f"redact_detections: image (offset {off}, {H}x{W}) outside the buffer or larger than "
                             f"{DRAW_MAX_SIDE} a side")
    if N == 0 or Q == 0:
        return buf_u8
    boxes, scores, labels, count = (t.contiguous() for t in (dets.boxes, dets.scores, dets.labels, dets.count))
    select = None if select is None else select.contiguous()
    fill = st["fill"]
    with torch.cuda.device(buf_u8.device):
        for i in range(0, N, PREPROCESS_BATCH_MAX):
            j = min(N, i + PREPROCESS_BATCH_MAX)
            work = None
            if st["mode"] == "blur":   # (launches on one stream run in order: the next group may reuse the workspace)
                need, key = _redact.work_bytes(rows[i:j], st["cell"]), str(buf_u8.device)
                work = _redact_work.get(key)
                if work is None or work.numel() < need:
                    work = _redact_work[key] = torch.empty((need,), dtype=torch.uint8, device=buf_u8.device)
            _redact.redact_detections(buf_u8, rows[i:j], boxes[i:j], scores[i:j], labels[i:j], count[i:j], select,
                                      _redact.MODES[st["mode"]], _redact.SHAPES[st["shape"]], st["cell"], st["score_thr"],
                                      st["expand"], (fill[0] << 16) | (fill[1] << 8) | fill[2], work)
    return buf_u8


JPEG_SETTINGS = dict(quality=90, subsampling="420")
JPEG_DOWNLOADS = {"copies": 0, "bytes": 0}   # device-to-host copies encode_jpeg made in this process


def jpeg_settings(settings=None):
    """quality / subsampling of encode_jpeg, validated: the keys of JPEG_SETTINGS (missing ones take its values) -> a new
    dict.  ValueError for an unknown key, a quality that is not an integer in 1..100, a subsampling other than '420' /
    '444'."""
    st = dict(JPEG_SETTINGS)
    settings = dict(settings or {})
    unknown = set(settings) - set(st)
    if unknown:
        raise ValueError(f"jpeg: unknown key(s) {sorted(unknown)}; known: {sorted(st)}")
    st.update(settings)
    q = st["quality"]
    if isinstance(q, bool) or not isinstance(q, (int, float)) or int(q) != q or not 1 <= q <= 100:
        raise ValueError(f"jpeg: quality must be an integer in 1..100, got {q!r}")
    if st["subsampling"] not in _jpeg.SUBSAMPLINGS:
        raise ValueError(f"jpeg: subsampling must be one of {sorted(_jpeg.SUBSAMPLINGS)}, got {st['subsampling']!r}")
    st["quality"] = int(q)
    return st


def jpeg_out_stride(rows, subsampling="420"):
    """the bytes encode_jpeg reserves per image of a launch group on its first attempt: an eighth of the largest raw image
    plus 4 KB, never more than the proven bound of the largest scan, rounded up to 16.  (A drawn 1080p frame at quality
    90 / 4:2:0 takes about a twentieth of its raw size; noise at quality 100 exceeds the raw size and takes the retry.)"""
    sub = _jpeg.SUBSAMPLINGS[subsampling]
    guess = max(H * W * 3 for _, H, W in rows) // 8 + 4096
    bound = max(_jpeg.scan_bound(H, W, sub) for _, H, W in rows)
    return (min(guess, bound) + 15) // 16 * 16


def encode_jpeg(src, rows, quality=90, subsampling="420", out_stride=None):
    """RGB images on the device -> complete baseline JPEG files, encoded on the GPU (csrc/jpeg.hip; the file is stated in
    include/codetr_jpeg.h): the scan comes from two launches per PREPROCESS_BATCH_MAX images, the header from the
    library's host builder.
      src       one flat uint8 device buffer holding RGB HWC images (the buffer draw_detections drew on)
      rows      (offset, H, W) per image
      quality   1..100 (the IJG scale); subsampling '420' | '444'
      out_stride  bytes reserved per image on the first attempt (default: jpeg_out_stride).  An image whose scan does not
                fit is encoded once more with the proven worst case reserved, in one launch group with the others that
                did not fit.
    -> list[bytes], one file per row.  One device-to-host copy per launch group: the int32 lengths and the slots travel
    in one buffer.  ValueError for a bad setting, a wrong dtype or shape, a CPU tensor, an image outside the buffer."""
    st = jpeg_settings(dict(quality=quality, subsampling=subsampling))
    if not torch.is_tensor(src) or not src.is_cuda:
        raise ValueError("encode_jpeg: src must be a tensor on a GPU")
    if src.dtype != torch.uint8 or src.dim() != 1 or not src.is_contiguous():
        raise ValueError("encode_jpeg: expected one contiguous flat uint8 buffer")
    rows = [tuple(int(v) for v in r) for r in rows]
    for off, H, W in rows:
        if not (1 <= H <= DRAW_MAX_SIDE and 1 <= W <= DRAW_MAX_SIDE) or off < 0 or off + H * W * 3 > src.numel():
            raise ValueError(f"encode_jpeg: image (offset {off}, {H}x{W}) outside the buffer or larger than "
                             f"{DRAW_MAX_SIDE} a side")
    if out_stride is not None and (int(out_stride) != out_stride or out_stride < 1):
        raise ValueError(f"encode_jpeg: out_stride must be a positive integer, got {out_stride!r}")
    sub = _jpeg.SUBSAMPLINGS[st["subsampling"]]
    scans = [None] * len(rows)

    def group(index, stride):
        """one launch group: encode rows[index] into slots of `stride` bytes -> the indices that did not fit"""
        part = [rows[i] for i in index]
        head = (4 * len(part) + 15) // 16 * 16   # the lengths lead the buffer, so that one copy brings both
        out = torch.empty((head + len(part) * stride,), dtype=torch.uint8, device=src.device)
        ws = torch.empty((_jpeg.workspace_bytes(part, sub, stride),), dtype=torch.uint8, device=src.device)
        _jpeg.encode(src, part, st["quality"], sub, out[head:], stride, out[:head].view(torch.int32), ws)
        host = out.cpu().numpy()
        JPEG_DOWNLOADS["copies"] += 1
        JPEG_DOWNLOADS["bytes"] += host.size
        lengths = host[:head].view(np.int32)
        missed = []
        for k, i in enumerate(index):
            if lengths[k] < 0:
                missed.append(i)
            else:
                scans[i] = host[head + k * stride:head + k * stride + int(lengths[k])].tobytes()
        return missed

    with torch.cuda.device(src.device):
        retry = []
        for i in range(0, len(rows), PREPROCESS_BATCH_MAX):
            index = list(range(i, min(len(rows), i + PREPROCESS_BATCH_MAX)))
            stride = int(out_stride) if out_stride is not None else jpeg_out_stride([rows[k] for k in index], st["subsampling"])
            retry += group(index, stride)
        for i in range(0, len(retry), PREPROCESS_BATCH_MAX):
            index = retry[i:i + PREPROCESS_BATCH_MAX]
            bound = max(_jpeg.scan_bound(rows[k][1], rows[k][2], sub) for k in index)
            if group(index, (bound + 15) // 16 * 16):
                raise RuntimeError("encode_jpeg: a scan exceeded its proven bound")
    return [_jpeg.header(H, W, st["quality"], sub) + scans[i] + b"\xff\xd9" for i, (_, H, W) in enumerate(rows)]


JPEG_DECODE_STATS = {"host_fallbacks": 0}   # files the GPU decoder does not support, decoded with Pillow on the host


def jpeg_file_bytes(item):
    """one JPEG file as a contiguous 1-D uint8 numpy array: bytes / bytearray / memoryview, a 1-D uint8 numpy array or
    host tensor, or a str / os.PathLike path"""
    if isinstance(item, (str, os.PathLike)):
        with open(item, "rb") as f:
            item = f.read()
    if isinstance(item, (bytes, bytearray, memoryview)):
        return np.frombuffer(item, np.uint8)
    if torch.is_tensor(item) and not item.is_cuda:
        item = item.detach().numpy()
    if isinstance(item, np.ndarray) and item.dtype == np.uint8 and item.ndim == 1:
        return np.ascontiguousarray(item)
    raise ValueError(f"jpeg: a file is bytes, a 1-D uint8 array or host tensor, or a path; got {type(item).__name__}")


def jpeg_parse(data):
    """the header of one file (a contiguous 1-D uint8 numpy array) -> (return code, info, tables) of
    codetr_jpegdec_parse; host only"""
    return _jpeg_dec.parse(data)


def jpeg_host_decode(data):
    """the file decoded on the host with Pillow -> RGB uint8 [H, W, 3], counted in JPEG_DECODE_STATS; None when Pillow
    does not import"""
    try:
        import io

        from PIL import Image
    except ImportError:
        return None
    rgb = np.asarray(Image.open(io.BytesIO(data.tobytes())).convert("RGB"))
    JPEG_DECODE_STATS["host_fallbacks"] += 1
    return rgb


def jpeg_reason(rc, info):
    if rc == 0:
        return None
    if rc == _cabi._D["CODETR_E_UNSUPPORTED"]:
        return _jpeg_dec.REASONS.get(int(info[6]), "unsupported")
    return "too_large" if rc == _cabi._D["CODETR_E_TOO_LARGE"] else "bad_header"


def jpeg_info(data):
    """What the header of a JPEG file says (host only; include/codetr_jpeg_dec.h's parser)
    -> dict(supported, reason, height, width, components, sampling [(h, v)], restart_interval, scan_offset, scan_bytes);
    reason: None, a name of the header's CODETR_JPEGDEC_R_* in lower case, 'too_large' or 'bad_header'; size and sampling
    are those of the frame header when it was read, else 0 / []."""
    rc, info, _ = _jpeg_dec.parse(jpeg_file_bytes(data))
    nc = int(info[2])
    return dict(supported=rc == 0, reason=jpeg_reason(rc, info), height=int(info[0]), width=int(info[1]), components=nc,
                sampling=[(int(info[9 + 5 * c]), int(info[10 + 5 * c])) for c in _range(min(nc, 3))] if nc in (1, 3) else [],
                restart_interval=int(info[3]), scan_offset=int(info[4]), scan_bytes=int(info[5]))


def jpeg_stage(parsed, pos=0):
    """Where the scans and tables of parsed files (file bytes, info, tables) go in a staging buffer, from byte `pos`:
    -> (copies [(offset, uint8 array)], per launch group of PREPROCESS_BATCH_MAX (index list, tables offset), end).  The
    scans lie back to back as they are in the files; a group's tables are contiguous and 16-byte aligned."""
    copies, groups, scan_at = [], [], []
    for data, info, _ in parsed:
        scan_at.append(pos)
        copies.append((pos, data[int(info[4]):int(info[4]) + int(info[5])]))
        pos += int(info[5])
    for i in _range(0, len(parsed), PREPROCESS_BATCH_MAX):
        index = list(_range(i, min(len(parsed), i + PREPROCESS_BATCH_MAX)))
        pos = -(-pos // 16) * 16
        groups.append((index, pos))
        for k in index:
            copies.append((pos, parsed[k][2]))
            pos += _jpeg_dec.TABLE_BYTES
    return copies, groups, scan_at, pos


def jpeg_decode_staged(up, parsed, groups, scan_at, dst_offsets, dst):
    """the decoder's launches behind the upload of a buffer laid out by jpeg_stage: image k of `parsed` goes to
    dst[dst_offsets[k]:] -> the int32 status words on the device, one per file (not fetched: no synchronisation)"""
    status = torch.empty((len(parsed),), dtype=torch.int32, device=up.device)
    with torch.cuda.device(up.device):
        for index, tables_at in groups:
            rows = [(scan_at[k], int(parsed[k][1][5]), int(parsed[k][1][0]), int(parsed[k][1][1]), dst_offsets[k]) for k in index]
            infos = np.stack([parsed[k][1] for k in index])
            ws = torch.empty((_jpeg_dec.workspace_bytes(rows, infos),), dtype=torch.uint8, device=up.device)
            _jpeg_dec.decode(up, rows, infos, up[tables_at:tables_at + len(index) * _jpeg_dec.TABLE_BYTES], dst,
                             status[index[0]:index[0] + len(index)], ws)
    return status


def jpeg_status_error(status, names):
    """ValueError naming the first file with a non-zero status word, or None; status: the words on the host"""
    for s, name in zip(status, names):
        if int(s) != 0:
            return ValueError(f"jpeg: {name}: the scan does not decode ({_jpeg_dec.STATUS.get(int(s), int(s))})")
    return None


def decode_jpeg(files, out=None, device="cuda:0"):
    """Baseline JPEG files -> packed RGB HWC images on the device, decoded on the GPU (csrc/jpeg_dec.hip; the rule and the
    supported files are stated in include/codetr_jpeg_dec.h): only the headers are read on the host, the scans are
    uploaded as they are in the files, in one copy with their tables, and decoded by five launches per
    PREPROCESS_BATCH_MAX files.
      files   each bytes / bytearray / memoryview, a 1-D uint8 array or host tensor, or a path
      out     a flat uint8 device buffer to decode into (at least the returned layout's bytes) instead of a new one
    -> (the flat uint8 buffer, [(offset, H, W)] per image); images start at multiples of 16 bytes, as stage_chunk lays
    them out.  ValueError naming the image and the reason for a bad header, a file outside the supported set, or a scan
    that does not decode."""
    if not len(files):
        raise ValueError("decode_jpeg: no files")
    parsed = []
    for i, item in enumerate(files):
        data = jpeg_file_bytes(item)
        rc, info, tables = _jpeg_dec.parse(data)
        if rc != 0:
            raise ValueError(f"decode_jpeg: image {i}: {jpeg_reason(rc, info)}")
        parsed.append((data, info, tables))
    staged, total = [], 0
    for _, info, _ in parsed:
        staged.append((total, int(info[0]), int(info[1])))
        total += _jpeg_dec.output_bytes(info[0], info[1])
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=device)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.numel() < total):
        raise ValueError(f"decode_jpeg: out must be a contiguous flat uint8 buffer of at least {total} bytes on a GPU")
    copies, groups, scan_at, end = jpeg_stage(parsed)
    staging = torch.empty((end,), dtype=torch.uint8, pin_memory=True)
    host = staging.numpy()
    for at, part in copies:
        host[at:at + part.size] = part
    up = staging.to(out.device, non_blocking=True)
    status = jpeg_decode_staged(up, parsed, groups, scan_at, [o for o, _, _ in staged], out)
    err = jpeg_status_error(status.cpu().numpy(), [f"image {i}" for i in _range(len(parsed))])
    if err is not None:
        raise err
    return out, staged


FRAME_FORMATS = _cabi.FRAME_FORMATS
FRAME_COLOR = dict(matrix="bt601", range="limited")   # what OpenCV's cvtColor(..., COLOR_YUV2RGB_NV12) computes
_range = range    # (frames_to_rgb has a parameter of that name)


def frames_to_rgb(src_u8, rows10, dst_bytes, matrix="bt601", range="limited", out=None):
    """Frames as decoders hand them out -> packed RGB HWC images in one new flat uint8 device buffer of `dst_bytes`
    bytes, one launch per PREPROCESS_BATCH_MAX frames (csrc/frames.hip; include/codetr_hip.h states the conversion).
      src_u8    one flat contiguous uint8 device buffer that holds every plane
      rows10    per frame (format, H, W, plane0_offset, plane0_pitch, plane1_offset, plane1_pitch, plane2_offset,
                plane2_pitch, dst_offset); format a name of FRAME_FORMATS or its code, offsets in bytes, the columns of
                a plane the format does not have 0
      matrix    'bt601' | 'bt709'; range 'limited' | 'full' (the YUV formats; ignored by the others)
      out       a flat uint8 buffer of dst_bytes on src_u8's GPU to write into instead of a new one (the frames of a
                chunk that lie in several source buffers: one call per source)
    -> the buffer; bytes outside the frames' images are not written.  ValueError for an unknown format, matrix or range
    and for a wrong dtype or shape; whatever else is inconsistent the entry point rejects before it launches."""
    _gpu(src_u8, "frames_to_rgb")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 1 or not src_u8.is_contiguous():
        raise ValueError("frames_to_rgb: expected one contiguous flat uint8 buffer")
    if matrix not in _cabi.COLOR_MATRICES or range not in _cabi.COLOR_RANGES:
        raise ValueError(f"frames_to_rgb: matrix one of {sorted(_cabi.COLOR_MATRICES)} and range one of "
                         f"{sorted(_cabi.COLOR_RANGES)}, got {matrix!r} / {range!r}")
    rows = []
    for r in rows10:
        if len(r) != 10:
            raise ValueError("frames_to_rgb: ten values per row (format, H, W, three (offset, pitch) pairs, dst_offset)")
        fmt = FRAME_FORMATS.get(r[0], r[0]) if isinstance(r[0], str) else r[0]
        if isinstance(fmt, str) or int(fmt) not in FRAME_FORMATS.values():
            raise ValueError(f"frames_to_rgb: unknown frame format {r[0]!r}; known: {sorted(FRAME_FORMATS)}")
        rows.append((int(fmt),) + tuple(int(v) for v in r[1:]))
    if not rows or int(dst_bytes) <= 0:
        raise ValueError("frames_to_rgb: no frames")
    if out is None:
        out = torch.empty((int(dst_bytes),), dtype=torch.uint8, device=src_u8.device)
    elif (not torch.is_tensor(out) or out.device != src_u8.device or out.dtype != torch.uint8 or out.dim() != 1
          or not out.is_contiguous() or out.numel() != int(dst_bytes)):
        raise ValueError("frames_to_rgb: out must be a contiguous flat uint8 buffer of dst_bytes on the source's GPU")
    dst = out
    with torch.cuda.device(src_u8.device):
        for i in _range(0, len(rows), PREPROCESS_BATCH_MAX):
            _cabi.frames_to_rgb(src_u8, rows[i:i + PREPROCESS_BATCH_MAX], _cabi.COLOR_MATRICES[matrix],
                                _cabi.COLOR_RANGES[range], dst)
    return dst


TRACK_MAX_TRACKS = _cabi.TRACK_MAX_TRACKS
# this build's defaults: mmdet's ByteTracker config values as recalled (unpinned: mmdet is not installed here); max_tracks
# is this build's own
TRACKER = dict(obj_score_thrs=dict(high=0.6, low=0.1), init_track_thr=0.7, weight_iou_with_det_scores=True,
               match_iou_thrs=dict(high=0.1, low=0.5, tentative=0.3), num_frames_retain=30, num_tentatives=3,
               max_tracks=256)
TrackState = collections.namedtuple("TrackState", "f next_id refused id label hits tentative last mean cov")


def track_settings(settings=None):
    """the settings of track_update, validated and completed from TRACKER (a partial obj_score_thrs / match_iou_thrs
    dict keeps the other defaults) -> a new dict.  ValueError for an unknown key, a threshold that is not a finite
    number, obj_score_thrs.low > high, num_frames_retain or num_tentatives < 1 or not an integer, max_tracks outside
    1..TRACK_MAX_TRACKS."""
    out = {k: dict(v) if isinstance(v, dict) else v for k, v in TRACKER.items()}
    settings = dict(settings or {})
    unknown = set(settings) - set(out)
    if unknown:
        raise ValueError(f"tracker: unknown key(s) {sorted(unknown)}; known: {sorted(out)}")

    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"tracker {name} must be a finite number, got {v!r}")
        return float(v)

    for key in ("obj_score_thrs", "match_iou_thrs"):
        if key in settings:
            given = settings[key]
            if not isinstance(given, dict) or set(given) - set(out[key]):
                raise ValueError(f"tracker {key}: a dict with keys of {sorted(out[key])}")
            out[key].update(given)
        out[key] = {k: number(f"{key}.{k}", v) for k, v in out[key].items()}
    if out["obj_score_thrs"]["low"] > out["obj_score_thrs"]["high"]:
        raise ValueError("tracker obj_score_thrs: low must not exceed high")
    out["init_track_thr"] = number("init_track_thr", settings.get("init_track_thr", out["init_track_thr"]))
    out["weight_iou_with_det_scores"] = bool(settings.get("weight_iou_with_det_scores", out["weight_iou_with_det_scores"]))
    for key, hi in (("num_frames_retain", 2 ** 31 - 1), ("num_tentatives", 2 ** 31 - 1), ("max_tracks", TRACK_MAX_TRACKS)):
        v = settings.get(key, out[key])
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError(f"tracker {key} must be an integer in 1..{hi}, got {v!r}")
        out[key] = v
    return out


def new_track_state(S, max_tracks, device):
    """the states of S fresh streams of max_tracks slots each: zeros [S, 16 + 104 max_tracks] uint8 on `device`
    (include/codetr_hip.h states the layout; track_state_to_host decodes it)"""
    if int(S) < 1:
        raise ValueError(f"new_track_state: at least one stream, got {S}")
    if not 1 <= int(max_tracks) <= TRACK_MAX_TRACKS:
        raise ValueError(f"new_track_state: max_tracks in 1..{TRACK_MAX_TRACKS}, got {max_tracks}")
    return torch.zeros((int(S), _cabi.track_state_bytes(max_tracks)), dtype=torch.uint8, device=device)


def _track_slots(state):
    if not torch.is_tensor(state) or state.dtype != torch.uint8 or state.dim() != 2 or not state.is_contiguous() or \
            state.shape[0] < 1 or state.shape[1] < 120 or (state.shape[1] - 16) % 104:
        raise ValueError("track state: a contiguous [S, 16 + 104 max_tracks] uint8 tensor (new_track_state)")
    return (state.shape[1] - 16) // 104


def track_state_to_host(state):
    """the states of new_track_state / track_update decoded on the host (one device-to-host copy) -> TrackState of numpy
    arrays: f, next_id, refused [S]; id, hits, tentative, last (int32) and label (int64) [S, T]; mean [S, T, 4, 2] (p, v of
    cx, cy, a, h) and cov [S, T, 4, 3] (A, B, C) float32"""
    T = _track_slots(state)
    raw = state.cpu().numpy()
    S = raw.shape[0]
    hdr = raw[:, :16].copy().view(np.int32)
    o = 16
    label = raw[:, o:o + 8 * T].copy().view(np.int64)
    o += 8 * T
    ints = raw[:, o:o + 16 * T].copy().view(np.int32).reshape(S, 4, T)
    o += 16 * T
    mean = raw[:, o:o + 32 * T].copy().view(np.float32).reshape(S, 4, 2, T).transpose(0, 3, 1, 2).copy()
    o += 32 * T
    cov = raw[:, o:o + 48 * T].copy().view(np.float32).reshape(S, 4, 3, T).transpose(0, 3, 1, 2).copy()
    return TrackState(hdr[:, 0].copy(), hdr[:, 1] + 1, hdr[:, 2].copy(), ints[:, 0].copy(), label, ints[:, 1].copy(),
                      ints[:, 2].copy(), ints[:, 3].copy(), mean, cov)


TRACK_ASSOCIATIONS = tuple(_assign.ASSOCIATIONS)   # "greedy" (the default, codetr_hip.h's rule) and "optimal"

# the appearance cue (include/codetr_appearance.h states the rule, these settings' ranges and the cue's limits).  The two
# thresholds are BoT-SORT's appearance_thresh (0.25, as a distance) and proximity_thresh as recalled (unpinned: BoT-SORT
# is not installed here); reid_gate is this library's own
APPEARANCE = dict(appearance_thr=0.75, proximity_thr=0.5, reid_gate=1.5)
APPEARANCE_BINS = _appearance.BINS


def appearance_settings(d=None):
    """the settings of the appearance cue, validated and completed from APPEARANCE -> a new dict.  ValueError for an
    unknown key or a value that is not a finite number of its range: the thresholds in [0, 1], reid_gate >= 0."""
    out = dict(APPEARANCE)
    d = dict(d or {})
    unknown = set(d) - set(out)
    if unknown:
        raise ValueError(f"appearance: unknown key(s) {sorted(unknown)}; known: {sorted(out)}")
    for key, hi in (("appearance_thr", 1.0), ("proximity_thr", 1.0), ("reid_gate", math.inf)):
        v = d.get(key, out[key])
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or \
                not 0 <= v <= hi:
            raise ValueError(f"appearance {key} must be a finite number in [0, {hi}], got {v!r}")
        out[key] = float(v)
    return out


_appearance_settings = appearance_settings   # (track_update has an argument of that name)


def appearance_descriptors(src_u8, rows, dets):
    """The colour descriptor of every detection in one launch per PREPROCESS_BATCH_MAX rows and without a synchronisation
    (csrc/appearance.hip; include/codetr_appearance.h states the rule: 16 x 32 samples over the inner three quarters of
    the box, two stripes of 64 two-bit RGB bins).
      src_u8  one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows    (offset, H, W) per image, one per row of the detections
      dets    Detections / SoftDetections over [N, Q] rows in source pixels (boxes and count are read)
    -> [N, Q, 128] int16 on the device (the header's uint16 bits: a value is at most 256); zeros for a row beyond count,
    with a non-finite coordinate or without area."""
    _gpu(src_u8, "appearance_descriptors")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 1 or not src_u8.is_contiguous():
        raise ValueError("appearance_descriptors: expected one contiguous flat uint8 buffer")
    boxes = dets.boxes
    if not torch.is_tensor(boxes) or boxes.dtype not in (torch.float16, torch.bfloat16, torch.float32) or \
            boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.device != src_u8.device:
        raise ValueError("appearance_descriptors: boxes [N, Q, 4] in f16, bf16 or f32 on the images' device")
    N, Q = boxes.shape[:2]
    rows = [tuple(int(v) for v in r) for r in rows]
    if len(rows) != N or tuple(dets.count.shape) != (N,):
        raise ValueError(f"appearance_descriptors: one image row and one count per detection row ({N})")
    for off, H, W in rows:
        if not (1 <= H <= _cabi.FRAME_MAX_SIDE and 1 <= W <= _cabi.FRAME_MAX_SIDE) or off < 0 or off + H * W * 3 > src_u8.numel():
            raise ValueError(f"appearance_descriptors: image (offset {off}, {H}x{W}) outside the buffer or larger than "
                             f"{_cabi.FRAME_MAX_SIDE} a side")
    if Q > _cabi.POSTPROCESS_MAX_Q:
        raise ValueError(f"appearance_descriptors: at most {_cabi.POSTPROCESS_MAX_Q} detection rows per frame, got {Q}")
    desc = torch.empty((N, Q, _appearance.BINS), dtype=torch.int16, device=src_u8.device)
    if N == 0 or Q == 0:
        return desc
    boxes, count = boxes.contiguous(), dets.count.contiguous()
    with torch.cuda.device(src_u8.device):
        for i in range(0, N, PREPROCESS_BATCH_MAX):
            j = min(N, i + PREPROCESS_BATCH_MAX)
            _appearance.describe(src_u8, rows[i:j], boxes[i:j], count[i:j], desc[i:j])
    return desc


def new_appearance_state(S, max_tracks, device):
    """the appearance states of S fresh streams of max_tracks slots each: zeros [S, max_tracks, 128] int16 on `device`
    (the header's uint16 in sixteenths; appearance_state_to_host decodes it)"""
    if int(S) < 1:
        raise ValueError(f"new_appearance_state: at least one stream, got {S}")
    if not 1 <= int(max_tracks) <= TRACK_MAX_TRACKS:
        raise ValueError(f"new_appearance_state: max_tracks in 1..{TRACK_MAX_TRACKS}, got {max_tracks}")
    return torch.zeros((int(S), int(max_tracks), _appearance.BINS), dtype=torch.int16, device=device)


def appearance_state_to_host(state):
    """the states of new_appearance_state / track_update on the host (one device-to-host copy) -> [S, T, 128] numpy
    uint16"""
    return state.cpu().numpy().view(np.uint16).copy()


def track_update(dets, state, streams=None, settings=None, association="greedy", motion=None, appearance=None,
                 appearance_state=None, appearance_settings=None):
    """Tracking-by-detection for the frames of a chunk in one launch per PREPROCESS_BATCH_MAX rows (track_kernel in
    csrc/track.hip, one kernel text instantiated per form of the update; the rule, modelled on mmdet's ByteTracker, is
    stated in include/codetr_hip.h): the three greedy associations, the Kalman filters, retirement and track starts of
    every stream on the device.
      dets      Detections / SoftDetections over [N, Q] rows, Q <= 1024: whatever the chunk's last launch produced
      state     new_track_state's tensor, updated in place; it stays on the device between calls
      streams   the state index in [0, S) of every row: one int for all rows, or one per row; None: 0.  The rows of a
                stream are its consecutive frames in row order (and from call to call)
      settings  the keys of TRACKER (track_settings); max_tracks must be the state's
      association  "greedy": the three greedy associations of codetr_hip.h; "optimal": each association is an assignment
                problem over integer gains, solved in the same launch (codetr_track_update2_*; the rule is stated in
                include/codetr_assign.h).  The state is the same: a stream may switch between calls
      motion    None, or estimate_motion's [N, 4] float32 (dx, dy, valid, 0 per row) on the detections' device: a valid,
                finite motion is added to the predicted centres of the row's live tracks before association
                (codetr_track_update3_*, include/codetr_motion.h).  None calls exactly the entry points it always did.
                Or estimate_motion(model="similarity")'s [N, 8] float32: by the row's model the similarity moves the
                predicted centres, their velocities and the height, or the translation is added (codetr_track_update4_*)
      appearance  None, or appearance_descriptors' [N, Q, 128] int16 of these detections: the first two associations add
                the colour similarity of track and candidate to the pair value, and a lost track inside the gate can match
                on it alone (codetr_track_update5_*, include/codetr_appearance.h).  A [N, 4] motion is widened on the
                device to [N, 8] with model = valid.  None calls exactly the entry points it always did.
      appearance_state     new_appearance_state's tensor for the same streams and max_tracks, updated in place; given
                exactly when `appearance` is
      appearance_settings  the keys of APPEARANCE (appearance_settings)
    -> [N, Q] int32 on the device: the id of the track each row updated or started, negated while the track is
    tentative, 0 for no track and beyond count."""
    cfg = track_settings(settings)
    if not isinstance(association, str) or association not in _assign.ASSOCIATIONS:
        raise ValueError(f"track_update: association must be one of {list(TRACK_ASSOCIATIONS)}, got {association!r}")
    scores = dets.scores
    _gpu(scores, "track_update")
    T = _track_slots(state)
    if state.device != scores.device:
        raise ValueError("track_update: the state lives on another device than the detections")
    if settings is not None and "max_tracks" in settings and cfg["max_tracks"] != T:
        raise ValueError(f"track_update: max_tracks {cfg['max_tracks']} but the state has {T} slots")
    if scores.dtype not in (torch.float16, torch.bfloat16, torch.float32) or dets.boxes.dtype != scores.dtype:
        raise ValueError("track_update: detections in f16, bf16 or f32")
    if scores.dim() != 2 or tuple(dets.boxes.shape) != tuple(scores.shape) + (4,):
        raise ValueError("track_update: boxes [N,Q,4], scores [N,Q], labels [N,Q], count [N]")
    N, Q = scores.shape
    if motion is not None:
        if not torch.is_tensor(motion) or motion.dtype != torch.float32 or \
                tuple(motion.shape) not in ((N, 4), (N, 8)) or motion.device != scores.device:
            raise ValueError("track_update: motion must be a [N, 4] or [N, 8] float32 tensor on the detections' device")
        motion = motion.contiguous()
    if (appearance is None) != (appearance_state is None):
        raise ValueError("track_update: appearance and appearance_state go together (appearance_descriptors, "
                         "new_appearance_state)")
    app_cfg = None
    if appearance is not None:
        app_cfg = _appearance_settings(appearance_settings)
        if not torch.is_tensor(appearance) or appearance.dtype != torch.int16 or \
                tuple(appearance.shape) != (N, Q, _appearance.BINS) or appearance.device != scores.device:
            raise ValueError(f"track_update: appearance must be a [N, Q, {_appearance.BINS}] int16 tensor on the "
                             "detections' device (appearance_descriptors)")
        if not torch.is_tensor(appearance_state) or appearance_state.dtype != torch.int16 or \
                appearance_state.dim() != 3 or not appearance_state.is_contiguous() or \
                appearance_state.device != scores.device or \
                tuple(appearance_state.shape) != (state.shape[0], T, _appearance.BINS):
            raise ValueError(f"track_update: appearance_state must be a contiguous [{state.shape[0]}, {T}, "
                             f"{_appearance.BINS}] int16 tensor on the detections' device (new_appearance_state)")
        appearance = appearance.contiguous()
        if motion is not None and motion.shape[1] == 4:   # model = valid: 1.0 adds the translation, 0.0 nothing
            motion = torch.cat([motion[:, :3], motion[:, 2:3], torch.zeros_like(motion)], dim=1).contiguous()
    streams = track_streams(streams, N)
    if any(v >= state.shape[0] for v in streams):
        raise ValueError(f"track_update: a stream index outside the state's {state.shape[0]} streams")
    if Q > _cabi.POSTPROCESS_MAX_Q:
        raise ValueError(f"track_update: at most {_cabi.POSTPROCESS_MAX_Q} detection rows per frame, got {Q}")
    ids = torch.zeros((N, Q), dtype=torch.int32, device=scores.device) if N == 0 or Q == 0 else \
        torch.empty((N, Q), dtype=torch.int32, device=scores.device)
    if N == 0 or Q == 0:
        return ids
    boxes, scores = dets.boxes.contiguous(), scores.contiguous()
    labels, count = dets.labels.contiguous(), dets.count.contiguous()
    thr = (cfg["obj_score_thrs"]["high"], cfg["obj_score_thrs"]["low"], cfg["init_track_thr"],
           cfg["match_iou_thrs"]["high"], cfg["match_iou_thrs"]["low"], cfg["match_iou_thrs"]["tentative"])
    with torch.cuda.device(scores.device):
        work = None
        if appearance is not None:
            work = torch.empty((_appearance.work_bytes(state.shape[0], T, Q),), dtype=torch.uint8, device=scores.device)
        for i in range(0, N, PREPROCESS_BATCH_MAX):
            j = min(N, i + PREPROCESS_BATCH_MAX)
            args = (boxes[i:j], scores[i:j], labels[i:j], count[i:j], streams[i:j], state, T, thr,
                    cfg["num_frames_retain"], cfg["num_tentatives"], cfg["weight_iou_with_det_scores"], ids[i:j])
            if appearance is not None:
                _appearance.track_update5(*args, _assign.ASSOCIATIONS[association], None if motion is None else motion[i:j],
                                          appearance[i:j], appearance_state,
                                          (app_cfg["appearance_thr"], app_cfg["proximity_thr"], app_cfg["reid_gate"]), work)
            elif motion is not None and motion.shape[1] == 8:
                _motion.track_update4(*args, _assign.ASSOCIATIONS[association], motion[i:j])
            elif motion is not None:
                _motion.track_update3(*args, _assign.ASSOCIATIONS[association], motion[i:j])
            elif association == "greedy":
                _cabi.track_update(*args)
            else:
                _assign.track_update2(*args, _assign.ASSOCIATIONS[association])
    return ids


# camera-motion compensation (include/codetr_motion.h states the rule and these settings' ranges)
MOTION = dict(grid=_motion.GRID_MAX, search=8, texture=2, min_blocks=4)
MOTION_MODELS = ("translation", "similarity")
MotionState = collections.namedtuple("MotionState", "have H W k thumb")


def motion_settings(d=None):
    """the settings of estimate_motion, validated and completed from MOTION -> a new dict.  ValueError for an unknown key or
    a value that is not an integer of its range: grid 32..160, search 1..16, texture 0..65535, min_blocks 1..100."""
    out = dict(MOTION)
    d = dict(d or {})
    unknown = set(d) - set(out)
    if unknown:
        raise ValueError(f"motion: unknown key(s) {sorted(unknown)}; known: {sorted(out)}")
    ranges = dict(grid=(_motion.GRID_MIN, _motion.GRID_MAX), search=(1, _motion.SEARCH_MAX),
                  texture=(0, _motion.TEXTURE_MAX), min_blocks=(1, _motion.MAX_BLOCKS))
    for key, (lo, hi) in ranges.items():
        v = d.get(key, out[key])
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"motion {key} must be an integer in {lo}..{hi}, got {v!r}")
        out[key] = int(v)
    return out


def new_motion_state(S, device):
    """the motion states of S fresh streams: zeros [S, 16 + 160 * 160] uint8 on `device` (int32 have, H, W, k, then the
    stream's last thumbnail; motion_state_to_host decodes it)"""
    if int(S) < 1:
        raise ValueError(f"new_motion_state: at least one stream, got {S}")
    return torch.zeros((int(S), _motion.state_bytes()), dtype=torch.uint8, device=device)


def motion_state_to_host(state):
    """the states of new_motion_state / estimate_motion on the host (one device-to-host copy) -> MotionState of numpy
    arrays: have, H, W, k [S] int32 and thumb [S, 160 * 160] uint8 (rows at pitch W // k, zero behind them)"""
    raw = state.cpu().numpy()
    hdr = raw[:, :16].copy().view(np.int32)
    return MotionState(hdr[:, 0].copy(), hdr[:, 1].copy(), hdr[:, 2].copy(), hdr[:, 3].copy(), raw[:, 16:].copy())


def estimate_motion(src_u8, rows, state, streams=None, settings=None, model="translation"):
    """The global image motion between the consecutive frames of every stream, in three launches per
    PREPROCESS_BATCH_MAX images and without a synchronisation (csrc/motion.hip; include/codetr_motion.h states the rule:
    block matching of gray thumbnails, a median vote, translation only).  model="similarity": five launches, the same
    votes fitted with a zoom and a roll as well (the header's version 2); the state is the same, so a stream may switch
    between the models from call to call.
      src_u8    one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows      (offset, H, W) per image
      state     new_motion_state's tensor, updated in place: it keeps every stream's last thumbnail between calls
      streams   the state index in [0, S) of every row, as track_update's
      settings  the keys of MOTION (motion_settings)
    -> (motion [N, 4] float32: dx, dy, valid (1.0 / 0.0), 0 -- scene content at p in the previous frame of the stream is
    at p + (dx, dy) in this one, in source pixels; diag [N, 4] int32: k, blocks, textured, agreeing), on the device.
    model="similarity" -> (motion [N, 8] float32: dx, dy, valid, model (2.0 similarity, 1.0 translation, 0.0 none), a, b,
    px, py -- content at p is at (px + dx, py + dy) + [[a, -b], [b, a]] (p - (px, py)); diag [N, 8] int32: the four above,
    eligible pairs, the best pair's inliers, its i, its j)."""
    if model not in MOTION_MODELS:
        raise ValueError(f"estimate_motion: model must be one of {list(MOTION_MODELS)}, got {model!r}")
    sim = model == "similarity"
    cfg = motion_settings(settings)
    _gpu(src_u8, "estimate_motion")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 1 or not src_u8.is_contiguous():
        raise ValueError("estimate_motion: expected one contiguous flat uint8 buffer")
    if not torch.is_tensor(state) or state.dtype != torch.uint8 or state.dim() != 2 or not state.is_contiguous() or \
            state.shape[0] < 1 or state.shape[1] != _motion.state_bytes():
        raise ValueError("estimate_motion: the state is a contiguous [S, 16 + 160 * 160] uint8 tensor (new_motion_state)")
    if state.device != src_u8.device:
        raise ValueError("estimate_motion: the state lives on another device than the images")
    rows = [tuple(int(v) for v in r) for r in rows]
    N = len(rows)
    for off, H, W in rows:
        if not (1 <= H <= _cabi.FRAME_MAX_SIDE and 1 <= W <= _cabi.FRAME_MAX_SIDE) or off < 0 or off + H * W * 3 > src_u8.numel():
            raise ValueError(f"estimate_motion: image (offset {off}, {H}x{W}) outside the buffer or larger than "
                             f"{_cabi.FRAME_MAX_SIDE} a side")
    streams = track_streams(streams, N)
    if any(v >= state.shape[0] for v in streams):
        raise ValueError(f"estimate_motion: a stream index outside the state's {state.shape[0]} streams")
    motion = torch.empty((N, 8 if sim else 4), dtype=torch.float32, device=src_u8.device)
    diag = torch.empty((N, 8 if sim else 4), dtype=torch.int32, device=src_u8.device)
    four = (cfg["grid"], cfg["search"], cfg["texture"], cfg["min_blocks"])
    with torch.cuda.device(src_u8.device):
        for i in range(0, N, PREPROCESS_BATCH_MAX):
            j = min(N, i + PREPROCESS_BATCH_MAX)
            nbytes = _motion.work2_bytes(j - i) if sim else _motion.work_bytes(j - i)
            work = torch.empty((nbytes,), dtype=torch.uint8, device=src_u8.device)
            if sim:
                _motion.estimate(src_u8, rows[i:j], streams[i:j], state, four, work, motion[i:j], diag[i:j], similarity=True)
            else:
                _motion.estimate(src_u8, rows[i:j], streams[i:j], state, four, work, motion[i:j], diag[i:j])
    return motion, diag


ASSIGN_MAX_ROWS, ASSIGN_MAX_COLS, ASSIGN_MAX_GAIN = _assign.MAX_ROWS, _assign.MAX_COLS, _assign.MAX_GAIN


def linear_assignment(gain):
    """Maximum-weight assignment of integer gains on the GPU, one workgroup per problem in one launch (csrc/assign.hip;
    the procedure and its tie rule are stated in include/codetr_assign.h, so the matches -- not just their total -- are
    reproducible): the shape of a DETR matcher, up to 512 targets x 1024 queries, after the caller has turned its costs
    into gains.
      gain  [n, m] or [B, n, m] int32 on a GPU, n <= ASSIGN_MAX_ROWS, m <= ASSIGN_MAX_COLS; values are clamped into
            [0, ASSIGN_MAX_GAIN]; a pair of gain 0 is never matched
    -> (match [.., n] int32: the column of every row, -1 for unmatched; total [..] int64: the sum of the matched gains)"""
    if not torch.is_tensor(gain) or gain.dtype != torch.int32 or gain.dim() not in (2, 3):
        raise ValueError("linear_assignment: gain must be an int32 tensor [n, m] or [B, n, m]")
    B, n, m = gain.shape if gain.dim() == 3 else (1,) + tuple(gain.shape)
    if n > ASSIGN_MAX_ROWS or m > ASSIGN_MAX_COLS:
        raise ValueError(f"linear_assignment: at most {ASSIGN_MAX_ROWS} rows x {ASSIGN_MAX_COLS} columns, got {n} x {m}")
    _gpu(gain, "linear_assignment")
    g = gain.contiguous().view(B, n, m)
    match = torch.full((B, n), -1, dtype=torch.int32, device=g.device)
    total = torch.zeros((B,), dtype=torch.int64, device=g.device)
    if B and n and m:
        with torch.cuda.device(g.device):
            for i in range(0, B, 65535):
                _assign.assign(g[i:i + 65535], match[i:i + 65535], total[i:i + 65535])
    return (match, total) if gain.dim() == 3 else (match[0], total[0])


def track_streams(streams, N):
    """the `streams` argument of track_update and Inferencer.__call__ -> a list of N non-negative ints: None is stream 0
    for every row, one int is that stream for every row; ValueError for anything else"""
    def one(v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"streams: non-negative integers, got {v!r}")
        return int(v)

    if streams is None:
        return [0] * N
    if isinstance(streams, (int, np.integer)):
        return [one(streams)] * N
    if not isinstance(streams, (list, tuple, np.ndarray)) or len(streams) != N:
        raise ValueError(f"streams: one non-negative integer, or one per frame ({N})")
    return [one(v) for v in streams]


def mask_pyramid(img_masks, shapes):
    """img_masks [B,H,W] (float 0/1, bool or uint8; non-zero = padding) + level shapes [(H_l, W_l)] ->
    (mask_flat [B,S] bool, ycum, xcum, valid_counts [B,L,2] fp32): the level masks (nearest resize), their running
    valid counts and first-row / first-column valid counts, one launch (csrc/mask_pyramid.hip).  ycum / xcum are flat
    fp32 buffers; `level_cums` slices out one level as [B,H_l,W_l]."""
    _gpu(img_masks, "mask_pyramid")
    m = img_masks
    if m.dtype not in (torch.bool, torch.uint8, torch.float16, torch.bfloat16, torch.float32):
        m = m != 0     # (other dtypes: one comparison kernel; the kernel tests the three element widths itself)
    with torch.cuda.device(m.device):
        return _cabi.mask_pyramid(m.contiguous(), [tuple(int(v) for v in s) for s in shapes])


def level_cums(ycum, xcum, B, start, hw):
    """level views [B,H_l,W_l] of mask_pyramid's running-count buffers (start = rows of the levels before)"""
    n = hw[0] * hw[1]
    return (ycum[B * start:B * (start + n)].view(B, hw[0], hw[1]), xcum[B * start:B * (start + n)].view(B, hw[0], hw[1]))


def sine_pos_tokens_into(mask, dest, row_start, level_embed, num_feats, temperature, scale, eps, offset, normalize,
                         cums=None):
    """Sine positional encoding of one level (mask [B,H,W] bool, True = padding) + level_embed, written into
    dest[:, row_start:row_start+H*W, :] (dest [B,S,2*num_feats] f16 contiguous).  cums = (ycum, xcum) [B,H,W] fp32
    from mask_pyramid skips the two cumsum calls (mask may then be None)."""
    if cums is None:
        _gpu(mask, "sine_pos_tokens_into")
        valid = ~mask
        ycum = valid.cumsum(1, dtype=torch.float32).contiguous()
        xcum = valid.cumsum(2, dtype=torch.float32).contiguous()
    else:
        ycum, xcum = cums
        _gpu(ycum, "sine_pos_tokens_into")
    if dest.dtype not in (torch.float16, torch.bfloat16) or not dest.is_contiguous() or dest.shape[2] != 2 * num_feats:
        raise AssertionError("destination must be a contiguous f16 / bf16 [B, S, 2*num_feats] tensor")
    if level_embed is not None and level_embed.dtype != dest.dtype:
        level_embed = level_embed.to(dest.dtype)
    with torch.cuda.device(ycum.device):
        _cabi.sine_pos_tokens(ycum, xcum, level_embed, dest[0, row_start:], dest.shape[1] * dest.shape[2], num_feats,
                              temperature, scale, eps, offset, normalize)
    return dest


def conv2d(x, weight, bias=None, stride=1, padding=0):
    _gpu(x, "conv2d")
    return F.conv2d(x, weight, bias, stride=stride, padding=padding)


def window_attention(qkv, rel_bias, mask, num_heads):
    """qkv [nWB, N, 3*C] (q|k|v, each head-major) ; rel_bias [nH, N, N]; mask [nW, N, N] or None.
    Returns [nWB, N, C].  softmax((q*scale) k^T + bias (+mask)) v per window and head
    (reference codetr/swin.py:92-112)."""
    _gpu(qkv, "window_attention")
    nWB, N, C3 = qkv.shape
    C = C3 // 3
    hd = C // num_heads
    qkv = qkv.view(nWB, N, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
    attn = attn + rel_bias.unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(nWB // nW, nW, num_heads, N, N) + mask[None, :, None]).view(nWB, num_heads, N, N)
    attn = attn.softmax(-1)
    return (attn @ v).transpose(1, 2).reshape(nWB, N, C)


def swin_window_attention_supported(x, embed_dims, num_heads, window_size):
    """True when the fused kernel serves this block (f16, head_dim 32, window in {4,7,8,12})."""
    return x.is_cuda and _cabi.window_attention_supported(x.dtype, embed_dims, num_heads, window_size)


WINDOW_BIAS_LANE = True   # route switch (A/B): False = the kernel reads the [nH, N, N] table as the reference lays it out
_LANE_INDEX = {}


def _rel_bias_lane_order(rel_bias, window_size):
    """rel_bias [nH, N, N] in the lane order of the window-attention kernel's score tiles (bias_layout 1 of
    codetr_window_attention_ex; same values, rows permuted along the key axis), cached on the table tensor; None where the
    window size has no lane order (7 x 7)."""
    if window_size not in _LANE_INDEX:
        _LANE_INDEX[window_size] = _cabi.window_attention_bias_index(window_size)
    idx = _LANE_INDEX[window_size]
    if idx is None:
        return None
    return derived((rel_bias,), "_codetr_rel_bias_lane",
                   lambda: rel_bias[..., torch.tensor(idx, dtype=torch.long, device=rel_bias.device)].contiguous())


def swin_window_attention(qkv, qkv_bias, rel_bias, hw_shape, num_heads, window_size, shift, out_scale=None, out_mx=False):
    """Fused (shifted-)window attention on the UNPADDED spatial token map.
    qkv [B, H*W, 3C] (output of the qkv Linear on real tokens only), qkv_bias [3C] or None,
    rel_bias [nH, N, N] -> [B, H*W, C].  Pad / roll / partition / softmax / reverse are all inside
    the kernel (reference codetr/swin.py:191-252, 92-112).
    out_scale (fp16 qkv only): the result is e4m3 = sat(f16(o) / out_scale), the operand of the fp8 proj GEMM;
    out_mx (fp16 qkv only): the result is (e4m3, MX block scales) -- one block per (token, head)."""
    _gpu(qkv, "swin_window_attention")
    B, L, C3 = qkv.shape
    H, W = hw_shape
    if L != H * W:
        raise AssertionError("input feature has wrong size")
    if not qkv.is_contiguous():
        qkv = qkv.contiguous()
    if qkv_bias is None:
        qkv_bias = torch.zeros(C3, dtype=qkv.dtype, device=qkv.device)
    if (out_scale is not None or out_mx) and qkv.dtype != torch.float16:
        raise ValueError("the e4m3 output forms take fp16 qkv")
    out = torch.empty((B, L, C3 // 3), dtype=FP8 if (out_scale is not None or out_mx) else qkv.dtype, device=qkv.device)
    scales = torch.empty(_cabi.mx_scale_bytes(B * L, C3 // 3), dtype=torch.uint8, device=qkv.device) if out_mx else None
    rel_bias = rel_bias.contiguous()
    lane = _rel_bias_lane_order(rel_bias, window_size) if WINDOW_BIAS_LANE else None
    with torch.cuda.device(qkv.device):
        _timed("window_attention", {"rows": B * L, "C": C3 // 3, "heads": num_heads, "window": window_size,
                                    "out_bytes": out.element_size()},
               lambda: _cabi.window_attention(qkv, qkv_bias, rel_bias if lane is None else lane, out, B, H, W, num_heads,
                                              window_size, shift, out_scale, scales, 0 if lane is None else 1), qkv.device)
    return (out, scales) if out_mx else out


def mha_self_attention(q, k, v, num_heads):
    """q,k,v [B, N, C] already projected (q / k may be column slices of one fused projection) -> [B, N, C]: dense
    softmax attention, 900 x 900 per head in the decoder (reference transformer_mmcv.py:394-428).  Native kernel for
    head_dim 32 and up to 1024 keys; the SDPA library call otherwise (fp32 parity runs, other head sizes)."""
    _gpu(q, "mha_self_attention")
    B, N, C = q.shape
    if _cabi.mha_attention_supported(q, k, v, num_heads):
        out = torch.empty((B, N, C), dtype=q.dtype, device=q.device)
        with torch.cuda.device(q.device):
            _cabi.mha_attention(q, k, v, num_heads, out)
        return out
    hd = C // num_heads
    sp = lambda t: t.reshape(B, -1, num_heads, hd).transpose(1, 2)  # noqa: E731
    o = F.scaled_dot_product_attention(sp(q), sp(k), sp(v))
    return o.transpose(1, 2).reshape(B, N, C)


def msda_fused_supported(value_dtype, head_dim, num_levels, num_points):
    return _cabi.msda_fused_supported(value_dtype, head_dim, num_levels, num_points)


def msda_head_major_supported(value_dtype, head_dim, num_levels, num_points):
    return _cabi.msda_head_major_supported(value_dtype, head_dim, num_levels, num_points)


def msda_fused(value, spatial_shapes, level_start_index, proj, off_col, logit_col, reference_points, num_levels,
               num_points, head_major=False):
    """MSDA with softmax + sampling-location arithmetic inside the kernel (reference
    multi_scale_deformable_attention.py:180-196 + the op).  value [B,S,M,D] (or [B,M,S,D] with head_major);
    proj [B,Nq,cols] = output of the fused (offsets | logits) projection; reference_points [B,Nq,L,2|4]
    -> [B,Nq,M*D]."""
    _gpu(value, "msda_fused")
    if head_major:
        B, M, S, D = value.shape
    else:
        B, S, M, D = value.shape
    out = torch.empty((B, proj.shape[1], M * D), dtype=value.dtype, device=value.device)
    ref32 = getattr(reference_points, "_codetr_ref32", None) if MSDA_FP32_REF else None
    ref = ref32 if ref32 is not None else reference_points.to(value.dtype).contiguous()
    if out.numel():
        with torch.cuda.device(value.device):
            _timed("msda_fused", {"B": B, "S": S, "Nq": proj.shape[1], "M": M, "D": D, "L": num_levels, "P": num_points},
                   lambda: _cabi.msda_fused(value.contiguous(), spatial_shapes, level_start_index, proj.contiguous(),
                                            off_col, logit_col, ref, num_levels, num_points, out,
                                            head_major=head_major), value.device)
    return out


def patch_embed_supported(x, weight, stride):
    kh, kw = weight.shape[-2:]
    return (x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and weight.dtype == x.dtype
            and kh == kw == 4 and tuple(stride) == (4, 4) and x.shape[1] * 16 <= 64 and not torch.is_grad_enabled())


def patch_embed(x, weight, bias):
    """PatchEmbed's Conv2d(C, E, 4, stride 4) with bottom / right zero padding as patch gather + GEMM: x [B,C,H,W] ->
    ([B, Hp*Wp, E] token-major, (Hp, Wp)).  The weight padded to 64 columns is cached on the parameter."""
    _gpu(x, "patch_embed")
    B, C, H, W = x.shape
    E = weight.shape[0]
    Hp, Wp = -(-H // 4), -(-W // 4)
    cache = getattr(weight, "_codetr_w64", None)
    if cache is None or cache[0] != weight._version or cache[1].device != weight.device:
        w64 = torch.zeros((E, 64), dtype=weight.dtype, device=weight.device)
        w64[:, :C * 16] = weight.detach().reshape(E, C * 16)
        cache = weight._codetr_w64 = (weight._version, w64)
    cols = torch.empty((B * Hp * Wp, 64), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _cabi.patch_im2col(x.contiguous(), 4, 64, cols)
    return linear(cols, cache[1], bias).view(B, Hp * Wp, E), (Hp, Wp)


def im2col_tokens(x4d, k, stride, pad):
    """k x k / stride / zero-pad patches of a token-major map x4d [B,H,W,C] -> [B, Ho*Wo, k*k*C], K ordered
    (ky, kx, c).  Native 16-byte gather for 16-bit maps with C % 8 == 0; strided slices + cat otherwise."""
    _gpu(x4d, "im2col_tokens")
    B, H, W, C = x4d.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if x4d.dtype in (torch.float16, torch.bfloat16) and C % 8 == 0:
        out = torch.empty((B, Ho * Wo, k * k * C), dtype=x4d.dtype, device=x4d.device)
        with torch.cuda.device(x4d.device):
            _cabi.im2col_tokens(x4d.contiguous(), k, stride, pad, out)
        return out
    xp = F.pad(x4d, (0, 0, pad, pad, pad, pad))
    return torch.cat([xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
                      for ky in range(k) for kx in range(k)], dim=-1).reshape(B, Ho * Wo, -1)


# ---- native ResNet-50 backbone (16-bit, token-major; codetr/resnet.py ResNet.forward_tokens) ----
R50_NATIVE = True        # route switch: False = 16-bit R50 models take the NCHW route (MIOpen / ATen convolutions)
R50_CONV_IM2COL = False  # A/B baseline: the 3x3 and strided 1x1 convs as codetr_im2col_tokens_b16 + codetr_linear_*


def conv_tokens(x4d, weight_kkc, bias, k, stride, pad, act=None, residual=None):
    """Conv2d(k, stride, pad) on a token-major map: x4d [B,H,W,C] -> [B,Ho,Wo,Cout] = act(conv + bias) (+ residual),
    weight_kkc [Cout, k*k*C] in (ky, kx, c) order; act as in linear ('relu_res': ReLU after the residual).  Native
    implicit-GEMM kernel; R50_CONV_IM2COL = True gathers the patches into a buffer and runs the linear instead."""
    _gpu(x4d, "conv_tokens")
    B, H, W, C = x4d.shape
    Cout = weight_kkc.shape[0]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if not _cabi.conv_tokens_supported(x4d, weight_kkc, k, stride, pad):
        raise RuntimeError(f"conv_tokens: no native kernel for x {tuple(x4d.shape)} {x4d.dtype}, k={k}, stride={stride}, "
                           f"pad={pad}, Cout={Cout} (C % 64 == 0, Cout % 8 == 0, k in (1, 3), stride in (1, 2))")
    if R50_CONV_IM2COL:
        cols = im2col_tokens(x4d, k, stride, pad)
        r = residual.reshape(B, Ho * Wo, Cout) if residual is not None else None
        return linear(cols, weight_kkc, bias, act=act, residual=r).view(B, Ho, Wo, Cout)
    x4d = x4d if x4d.is_contiguous() else x4d.contiguous()
    if residual is not None and not residual.is_contiguous():
        residual = residual.contiguous()
    out = torch.empty((B, Ho, Wo, Cout), dtype=x4d.dtype, device=x4d.device)
    with torch.cuda.device(x4d.device):
        _timed("conv_tokens", {"M": B * Ho * Wo, "N": Cout, "K": k * k * C},
               lambda: _cabi.conv_tokens(x4d, weight_kkc, bias, residual, k, stride, pad, act, out), x4d.device)
    return out


def stem_conv_tokens(x, weight_pad, bias, k, stride, pad):
    """relu(Conv2d(C, Cout, k, stride, pad)(x) + bias) on the NCHW image as window gather + native GEMM:
    x [B,C,H,W] 16-bit -> [B,Ho,Wo,Cout]; weight_pad [Cout, kpad] = conv.weight.view(Cout, C*k*k) zero-padded"""
    _gpu(x, "stem_conv_tokens")
    B, C, H, W = x.shape
    Cout, kpad = weight_pad.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = torch.empty((B * Ho * Wo, kpad), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _cabi.conv_im2col_nchw(x if x.is_contiguous() else x.contiguous(), k, stride, pad, kpad, cols)
    return linear(cols, weight_pad, bias, act="relu").view(B, Ho, Wo, Cout)


def maxpool_tokens(x4d):
    """F.max_pool2d(x, 3, 2, 1) on a 16-bit token-major map [B,H,W,C] (C % 8 == 0) -> [B,Ho,Wo,C]"""
    _gpu(x4d, "maxpool_tokens")
    B, H, W, C = x4d.shape
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=x4d.dtype, device=x4d.device)
    with torch.cuda.device(x4d.device):
        _cabi.maxpool_tokens(x4d if x4d.is_contiguous() else x4d.contiguous(), out)
    return out


# (The library routes these three ops can also take -- SDPA, the MIOpen stem convolution, torch.topk -- were measured
# against the native kernels in rounds 1-2 and are no longer selectable here: tools/ab_library_routes.py times them by
# patching this module from the outside.  What remains below them is the route for shapes / dtypes the kernels do not
# take: fp32 parity runs, other head sizes.)


def topk(x, k, want_values=True):
    """torch.topk(x, k, dim=-1) for the head's two selections (reference transformer.py:560-561, co_dino_head.py:183):
    (values, indices), sorted descending; ties by ascending index and NaN first on the native path (f16 / bf16 rows,
    k <= 1024), torch.topk otherwise (fp32 parity runs)."""
    _gpu(x, "topk")
    x2 = x.reshape(-1, x.shape[-1])
    if not torch.is_grad_enabled():
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        if _cabi.topk_supported(x2, k):
            idx = torch.empty((x2.shape[0], k), dtype=torch.int64, device=x.device)
            val = torch.empty((x2.shape[0], k), dtype=x.dtype, device=x.device) if want_values else None
            with torch.cuda.device(x.device):
                _cabi.topk(x2, k, val, idx)
            shape = (*x.shape[:-1], k)
            return (val.view(shape) if val is not None else None), idx.view(shape)
    v, i = torch.topk(x, k, dim=-1)
    return v, i


# Route switches of the encoder MSDA (plain module attributes; tools/ab_host_routes.py patches them for A/B runs -- the
# package reads no CODETR_* environment variable except checkpoint.py's CODETR_ALLOW_PICKLE):
MSDA_ENCODER = True     # False = general fused kernel in the encoder
MSDA_FP32_REF = True    # False = reference points read in the model dtype


_SWITCH_DEFAULTS = {"ENC_POSGEN": True, "WINDOW_BIAS_LANE": True, "LINEAR_PP": True, "SWIN_MLP": True, "SWIN_MLP_MIN_ROWS": 32768, "LN_GEMM": True, "XADD": True, "XADD_MIN_ROWS": 0, "MERGE_LN": True, "MSDA_ENCODER": True,
                    "MSDA_FP32_REF": True, "FP8_MIN_TILES": 96,
                    "R50_NATIVE": True, "R50_CONV_IM2COL": False}


def nondefault_switches():
    """Names of the host package's route switches that are not at their default (the measured-best path): the plan
    exporter refuses to record under any of them, tools/ab_host_routes.py sets them."""
    import sys

    from . import multi_scale_deformable_attention as msda_mod
    from . import transformer as tr_mod

    me = sys.modules[__name__]
    out = [k for k, v in _SWITCH_DEFAULTS.items() if getattr(me, k) != v]
    if msda_mod.HEAD_MAJOR_VALUE:
        out.append("HEAD_MAJOR_VALUE")
    out += [k for k in ("DEC_FUSED", "DEC_VPROJ") if not getattr(tr_mod, k)]
    return sorted(out)


# ---- round-5 encoder kernel (csrc/msda_encoder4.hip): lane-major packed projection, scalar geometry, zero border ----
MSDA_V4 = True                 # route switch: False = the general fused kernel on the unpacked projection
# Measured on MI355X at 4 x 1920x1280, offsets with 0 / 2 / 4 / 8 px of spread (profiles/r05_msda_encoder4_sweep.txt):
# 512 threads x 16x16 regions x 64 KiB = 918 / 973 / 1210 / 1637 us per launch; 256 x 16x8 x 40 KiB = 926 / 1019 / 1332 /
# 1832; 80 KiB windows trade 3 % at 2 px for 5 % at 8 px (round-4 kernel: 1220 / 1318 / 1810 / 2566).
MSDA_V4_THREADS = 512          # workgroup size (256: four workgroups per CU; 512: two)
MSDA_V4_REGION = (16, 16)      # region of a workgroup, pixels of the finest level
MSDA_V4_LDS_BUDGET = 64 * 1024   # bytes per workgroup
MSDA_V4_MARGIN_CAP = 40.0      # pixels: windows grow up to this margin around a head's bias points within the LDS budget
MSDA_V4_HEAD_MAJOR = True      # value projection writes [B, M, S, 32] for the packed encoder kernel
ENC_PROJ_FUSED = True          # value projection and packed (offsets | logits) projection as ONE launch (x, pos read once)
_SWITCH_DEFAULTS.update({"MSDA_V4": True, "MSDA_V4_THREADS": 512, "MSDA_V4_REGION": (16, 16),
                         "MSDA_V4_LDS_BUDGET": 64 * 1024, "MSDA_V4_MARGIN_CAP": 40.0,
                         "MSDA_V4_HEAD_MAJOR": True, "ENC_PROJ_FUSED": True, "FFN_OPROJ": True})


def msda_encoder_packed_supported(dtype, head_dim, num_levels, num_points):
    return (MSDA_V4 and MSDA_ENCODER and dtype in (torch.float16, torch.bfloat16) and head_dim == 32 and num_levels == 5
            and num_points == 4)


def value_projection_f16(x, weight, bias, row_mask, head_dim):
    """bf16 model: the encoder MSDA's value projection with an FP16, head-major result [B, M, S, head_dim] (the packed
    kernel's value map is fp16 whatever the model's type).  None when the library has no kernel for the shape."""
    _gpu(x, "value_projection_f16")
    if not (x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and x.dim() == 3):
        return None
    B, S, K = x.shape
    N = weight.shape[0]
    x2 = x.reshape(-1, K)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    w = weight if weight.is_contiguous() else weight.contiguous()
    mk = None
    if row_mask is not None:
        mk = row_mask.reshape(-1)
        if mk.dtype != torch.bool and mk.dtype != torch.uint8:
            mk = mk != 0
        mk = mk.contiguous()
    out = torch.empty((B * S, N), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        ok = _cabi.linear_bf16_f16out(x2, w, bias, out, mk, S, int(head_dim))
    return out.view(B, N // head_dim, S, head_dim) if ok else None


ENC_POSGEN = True   # route switch (A/B): False = the encoder's projections read the positional encoding tensor


def encoder_projections(x, pos, w_cat, b_cat, row_mask, n_value, head_dim):
    """The encoder self-attention's value projection and packed (offsets | logits) projection as ONE launch
    (include/codetr_hip.h codetr_encoder_projections_*; reference multi_scale_deformable_attention.py:161-182 with
    value = query): value = x @ w_cat[:n_value]^T + b (rows where row_mask is True zeroed), returned head-major
    [B, n_value / head_dim, S, head_dim] in FP16 (fp16 and bf16 models alike: the packed MSDA kernel's value map), and
    packed [B, S, Np] = (x + pos) @ w_cat[n_value:]^T + b in x's type.  None where the library declines the shape (the
    caller then runs the two GEMMs)."""
    _gpu(x, "encoder_projections")
    if not (ENC_PROJ_FUSED and x.dim() == 3 and x.dtype in (torch.float16, torch.bfloat16) and pos is not None
            and pos.shape == x.shape and pos.dtype == x.dtype and w_cat.dtype == x.dtype and not torch.is_grad_enabled()):
        return None
    B, S, K = x.shape
    n_packed = w_cat.shape[0] - n_value
    x2, p2 = x.reshape(-1, K), pos.reshape(-1, K)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    p2 = p2 if p2.is_contiguous() else p2.contiguous()
    mk = None
    if row_mask is not None:
        mk = row_mask.reshape(-1)
        if mk.dtype != torch.bool and mk.dtype != torch.uint8:
            mk = mk != 0
        mk = mk.contiguous()
    value = torch.empty((B * S, n_value), dtype=torch.float16, device=x.device)
    packed = torch.empty((B * S, n_packed), dtype=x.dtype, device=x.device)
    gen = getattr(pos, "_codetr_posgen", None) if ENC_POSGEN else None   # (set by the producer of `pos`: co_dino_head.py)

    def launch():
        if gen is not None and gen["S"] == S and gen["B"] == B:
            if _cabi.encoder_projections_posgen(x2, S, gen["cums"], gen["shapes"], gen["level_embed"], gen["temperature"],
                                                gen["scale"], gen["eps"], gen["offset"], gen["normalize"], w_cat, b_cat,
                                                mk, value, packed, S, int(head_dim)):
                return True
        return _cabi.encoder_projections(x2, p2, w_cat, b_cat, mk, value, packed, S, int(head_dim))

    with torch.cuda.device(x.device):
        ok = _timed_linear(launch, x.device, B * S, n_value + n_packed, K)
    if not ok:
        return None
    return value.view(B, n_value // head_dim, S, head_dim), packed.view(B, S, n_packed)


def msda_packed_projection(w_off, b_off, w_aw, b_aw, num_heads, num_levels, num_points):
    """(sampling_offsets | attention_weights) as ONE [64 M, C] weight + [64 M] bias whose output row is the lane-major
    packed layout codetr_msda_encoder_forward_packed_f16 reads (include/codetr_hip.h): per head 4 x 16 columns = the
    (x, y) offsets of point p on the five levels, its five logits, one zero pad column.  Pure row permutation of the
    reference's two Linears (multi_scale_deformable_attention.py:83-85): no arithmetic changes."""
    idx = _cabi.msda_pack_projection_index(num_heads, num_levels, num_points)
    if idx is None:
        return None
    ii = torch.tensor(idx, dtype=torch.long, device=w_off.device)
    wcat = torch.cat((w_off, w_aw), 0)
    bcat = torch.cat((b_off, b_aw), 0)
    pad = ii < 0
    wp = wcat[ii.clamp_min(0)].clone()
    bp = bcat[ii.clamp_min(0)].clone()
    wp[pad] = 0
    bp[pad] = 0
    return wp.contiguous(), bp.contiguous()


def msda_encoder_windows_packed(bias, level_shapes, num_heads, num_levels, num_points):
    """Staged window per (head, level) for the packed encoder kernel, as msda_encoder_windows: the bounding box of the
    head's bias points on that level grown by the largest margin (steps of 1/2 pixel, at most MSDA_V4_MARGIN_CAP) that
    keeps the workgroup inside MSDA_V4_LDS_BUDGET, per pass {0}, {1, 2}, {3, 4}.  Windows are clamped to the level (plus
    its zero border) by the kernel, so on the coarse levels a generous margin ends as whole-level residency."""
    import math

    b = bias.detach().float().cpu().view(num_heads, num_levels, num_points, 2)
    b = torch.round(b * 1024) / 1024
    lo, hi = b.amin(2).tolist(), b.amax(2).tolist()
    groups = [[0], [1, 2], [3, 4]]
    steps = int(2 * MSDA_V4_MARGIN_CAP)

    def window(m, l, mg):
        return (max(-127, math.floor(lo[m][l][0] - mg)), min(127, math.ceil(hi[m][l][0] + mg)),
                max(-127, math.floor(lo[m][l][1] - mg)), min(127, math.ceil(hi[m][l][1] + mg)))

    def need(trial):
        return _cabi.msda_encoder_packed_lds_bytes(level_shapes, num_heads, num_points, [trial] * num_heads,
                                                   MSDA_V4_REGION, MSDA_V4_THREADS)

    out = []
    for m in range(num_heads):
        win = [window(m, l, 0.0) for l in range(num_levels)]
        for grp in groups:
            a, z = 0, steps          # largest half-step count that fits (monotone): bisection
            while a < z:
                mid = (a + z + 1) // 2
                trial = list(win)
                for l in grp:
                    trial[l] = window(m, l, 0.5 * mid)
                n = need(trial)
                if 0 < n <= MSDA_V4_LDS_BUDGET:
                    a = mid
                else:
                    z = mid - 1
            for l in grp:
                win[l] = window(m, l, 0.5 * a)
        out.append(win)
    return out


def msda_encoder_packed(value, level_shapes, packed, num_points, windows, valid_counts, head_major=False):
    """Encoder self-attention MSDA on the lane-major packed projection (round-5 kernel).  value [B,S,M,32] fp16 (or
    [B,M,S,32] with head_major: what linear(..., head_major=32) returns), packed [B,S,64 M] fp16, valid_counts [B,L,2]
    fp32.  Returns None when the library does not take the shape."""
    _gpu(value, "msda_encoder_packed")
    if head_major:
        B, M, S, D = value.shape
    else:
        B, S, M, D = value.shape
    if not (valid_counts is not None and valid_counts.dtype == torch.float32 and valid_counts.is_contiguous()
            and valid_counts.shape == (B, len(level_shapes), 2) and packed.shape[:2] == (B, S) and packed.is_contiguous()):
        return None
    if value.dtype != torch.float16 or packed.dtype not in (torch.float16, torch.bfloat16):
        return None
    out = torch.empty((B, S, M * D), dtype=packed.dtype, device=value.device)
    ok = [True]

    def run():
        ok[0] = _cabi.msda_encoder_packed(value.contiguous(), level_shapes, packed, num_points, windows, valid_counts,
                                          MSDA_V4_REGION, MSDA_V4_THREADS, out, head_major)

    with torch.cuda.device(value.device):
        _timed("msda_fused", {"B": B, "S": S, "Nq": S, "M": M, "D": D, "L": len(level_shapes), "P": num_points},
               run, value.device)
    return out if ok[0] else None


def msda(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step):
    """The reference's native op, hand-written HIP behind the C ABI (always native)."""
    return torch.ops.codetr.multi_scale_deformable_attention(
        value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step
    )


# ---------------------------------------------------------------------------------------------------------------
# fp8 (OCP e4m3) path -- BASELINE config 5.  Weights are quantised once per parameter (per-output-channel scales),
# activations with static per-tensor scales from a calibration forward (codetr/fp8.py); fp32 accumulation.
# ---------------------------------------------------------------------------------------------------------------
FP8 = _cabi.FP8
FP8_MAX = 448.0
FP8_MIN_TILES = 96   # 256x256 output tiles below which fp16 serves the layer


def fp8_weight(weight):
    """(w8 [N,K] e4m3, w_scale [N] fp32) of an nn.Linear weight: per-output-channel absmax / 448; cached on the parameter"""
    def build():
        w = weight.detach().float()
        scale = (w.abs().amax(1) / FP8_MAX).clamp_min(1e-12)
        return (w / scale[:, None]).to(FP8).contiguous(), scale.contiguous()

    return derived((weight,), "_codetr_fp8_w", build)


def ffn_fp8_supported(x, w1, w2, act):
    """the fp8 fused FFN serves the same layers as ffn_fused with hidden a multiple of 128 (<= 2048), fp16 storage"""
    return (ffn_fused_supported(x, w1, w2, act) and x.dtype == torch.float16 and w1.shape[0] % 128 == 0
            and w1.shape[0] <= 2048)


def ffn_fp8_weights(w1, w2):
    """(w1q [hidden,256] e4m3, s1 [hidden], w2q_packed [256,hidden] e4m3, s2 [256]) of an FFN's two Linear weights:
    per-row absmax / 448 scales; W2's columns permuted inside every 128-block into the order in which the first
    product's accumulators become the second product's operand (packed column 32 g + 4 t + r <- unit 16 t + 4 g + r).
    Cached on w1."""
    def build():
        a, b = w1.detach().float(), w2.detach().float()
        s1 = (a.abs().amax(1) / FP8_MAX).clamp_min(1e-12)
        s2 = (b.abs().amax(1) / FP8_MAX).clamp_min(1e-12)
        p = torch.arange(128, device=w2.device)
        g, t, r = p // 32, (p % 32) // 4, p % 4
        src = 16 * t + 4 * g + r
        bq = (b / s2[:, None]).to(FP8).view(torch.uint8).view(b.shape[0], -1, 128)[:, :, src].reshape(b.shape).contiguous()
        return (a / s1[:, None]).to(FP8).contiguous(), s1.contiguous(), bq.view(FP8), s2.contiguous()

    return derived((w1, w2), "_codetr_ffn_fp8_w", build)


def ffn_fp8(x, w1, b1, w2, b2, x_scale, h_scale, ln=None, pos=None, ln_in=None):
    """ffn_fused on the e4m3 matrix path: both products in fp8 with static activation scales (x_scale for the -- possibly
    LayerNorm'ed -- input, h_scale for the hidden activation), fp16 in and out; same epilogue options."""
    _gpu(x, "ffn_fp8")
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    out = torch.empty_like(x2)
    p2 = out2 = None
    if pos is not None:
        p2 = pos.reshape(-1, pos.shape[-1])
        if p2.shape != x2.shape or p2.dtype != x2.dtype:
            raise ValueError("pos must match x in shape and dtype")
        if not p2.is_contiguous():
            p2 = p2.contiguous()
        out2 = torch.empty_like(x2)
    w1q, s1, w2q, s2 = ffn_fp8_weights(w1, w2)
    if x2.shape[0] > 0:
        with torch.cuda.device(x.device):
            _timed("ffn_fp8", {"M": x2.shape[0], "C": x2.shape[1], "hidden": w1.shape[0]},
                   lambda: _cabi.ffn_fp8(x2, w1q, s1, b1, w2q, s2, b2, out, x_scale, h_scale, ln, p2, out2, ln_in), x.device)
    if pos is not None:
        return out.view(x.shape), out2.view(x.shape)
    return out.view(x.shape)


def linear_fp8_supported(rows, weight):
    """True when the fp8 GEMM serves this layer: K a multiple of 128 bytes, N of 8, and enough 256x256 output tiles to
    fill the chip (smaller problems stay on the fp16 kernels)"""
    N, K = weight.shape
    return (weight.is_cuda and weight.dtype == torch.float16 and K % 128 == 0 and N % 8 == 0
            and -(-rows // 256) * -(-N // 256) >= FP8_MIN_TILES
            and rows * N <= 0x7fffffff)   # (the kernel's 32-bit output offsets: larger batches stay on the fp16 kernels)


def linear_fp8(x8, x_scale, weight, bias=None, act=None, residual=None, out_scale=None):
    """act((x8 * x_scale) @ weight.T + bias) (+ residual) with x8 e4m3 [..., K] and the fp16 `weight` quantised per
    output channel (cached).  Returns fp16, or e4m3 = sat(y / out_scale) when out_scale is given."""
    _gpu(x8, "linear_fp8")
    w8, ws = fp8_weight(weight)
    K, N = x8.shape[-1], weight.shape[0]
    x2 = x8.reshape(-1, K)
    r2 = None if residual is None else residual.reshape(-1, N).contiguous()
    out = torch.empty((x2.shape[0], N), dtype=FP8 if out_scale is not None else torch.float16, device=x8.device)
    with torch.cuda.device(x8.device):
        launch = lambda: _cabi.linear_fp8(x2, w8, ws, x_scale, bias, r2, act, out, out_scale or 0.0)  # noqa: E731
        _timed_linear(launch, x8.device, x2.shape[0], N, K, "fp8")
    return out.view(*x8.shape[:-1], N)


def linear_fp8mx(x8, x_scales, weight, bias=None, act=None, residual=None, out_mx=False):
    """act((x8 (*) block scales) @ weight.T + bias) (+ residual): x8 e4m3 [..., K] with its MX scale tensor, the fp16
    `weight` quantised per output channel (cached).  Returns fp16, or (e4m3, scales) with block scales along N."""
    _gpu(x8, "linear_fp8mx")
    w8, ws = fp8_weight(weight)
    K, N = x8.shape[-1], weight.shape[0]
    x2 = x8.reshape(-1, K)
    r2 = None if residual is None else residual.reshape(-1, N).contiguous()
    out = torch.empty((x2.shape[0], N), dtype=FP8 if out_mx else torch.float16, device=x8.device)
    sy = torch.empty(_cabi.mx_scale_bytes(x2.shape[0], N), dtype=torch.uint8, device=x8.device) if out_mx else None
    with torch.cuda.device(x8.device):
        launch = lambda: _cabi.linear_fp8mx(x2, x_scales, w8, ws, bias, r2, act, out, sy)  # noqa: E731
        _timed_linear(launch, x8.device, x2.shape[0], N, K, "fp8")
    out = out.view(*x8.shape[:-1], N)
    return (out, sy) if out_mx else out


def cast_fp8mx(x):
    """fp16 [..., C] -> (e4m3, MX block scales), C % 128 == 0"""
    _gpu(x, "cast_fp8mx")
    x2 = x.reshape(-1, x.shape[-1])
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    out = torch.empty(x2.shape, dtype=FP8, device=x.device)
    sy = torch.empty(_cabi.mx_scale_bytes(*x2.shape), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _cabi.cast_fp8mx(x2, out, sy)
    return out.view(x.shape), sy


def layer_norm_fp8mx(x, weight, bias, eps):
    """LayerNorm(x) -> (e4m3, MX block scales) in one kernel (fp16 input; the norm's fp16 output is never written)"""
    _gpu(x, "layer_norm_fp8mx")
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    out = torch.empty(x2.shape, dtype=FP8, device=x.device)
    sy = torch.empty(_cabi.mx_scale_bytes(x2.shape[0], C), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _cabi.layernorm_fp8mx(x2, weight, bias, eps, out, sy)
    return out.view(x.shape), sy


def mx_dequant(x8, scales):
    """(tests / diagnostics) the fp32 values an (e4m3, MX scales) pair stands for"""
    x2 = x8.reshape(-1, x8.shape[-1])
    M, K = x2.shape
    m = torch.arange(M, device=x8.device)[:, None]
    kb = torch.arange(K // 32, device=x8.device)[None, :]
    MB = -(-M // 128)
    idx = ((((kb >> 2) * MB + (m >> 7)) * 64 + (kb & 3) * 16 + (m & 15)) * 8 + ((m >> 4) & 7)).long()
    e = scales.long()[idx].float() - 127.0                       # [M, K / 32]
    return (x2.float().view(M, K // 32, 32) * torch.exp2(e)[:, :, None]).view(x8.shape)


def cast_fp8(x, scale):
    """sat(x / scale) -> e4m3, fp16 input"""
    _gpu(x, "cast_fp8")
    x = x if x.is_contiguous() else x.contiguous()
    out = torch.empty(x.shape, dtype=FP8, device=x.device)
    with torch.cuda.device(x.device):
        _cabi.cast_fp8(x, scale, out)
    return out


def layer_norm_fp8(x, weight, bias, eps, scale):
    """sat(LayerNorm(x) / scale) -> e4m3 in one kernel (fp16 input; the norm's fp16 output is never written)"""
    _gpu(x, "layer_norm_fp8")
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    out = torch.empty(x2.shape, dtype=FP8, device=x.device)
    with torch.cuda.device(x.device):
        _cabi.layernorm_fp8(x2, weight, bias, eps, scale, out)
    return out.view(x.shape)


# ---------------------------------------------------------------------------------------------------------------
# small element-wise / gather kernels of the decoder and the head (csrc/small_ops.hip); the torch formulation serves
# fp32 / bf16 parity runs and autograd
# ---------------------------------------------------------------------------------------------------------------
def _native16(*ts):
    return ((not torch.is_grad_enabled()) and ts[0].dtype in (torch.float16, torch.bfloat16)
            and all(t.is_cuda and t.dtype == ts[0].dtype and t.data_ptr() % 16 == 0 for t in ts))


def add(a, b):
    """a + b for same-shape fp16 tensors, or `a` broadcast over b's leading dimension (a stride-0 batch view of a
    parameter, e.g. query_embed.weight[None].expand(B, ...)): `query + query_pos` of the attention layers"""
    _gpu(b, "add")
    if _native16(a, b) and a.shape == b.shape and b.is_contiguous() and b.numel() % 8 == 0:
        period = None
        if a.is_contiguous():
            period = b.numel()
        elif a.dim() >= 2 and a.stride(0) == 0 and a[0].is_contiguous() and a[0].numel() % 8 == 0:
            period = a[0].numel()
        if period is not None:
            out = torch.empty_like(b)
            with torch.cuda.device(b.device):
                _cabi.add_f16(a, b, out, period)
            return out
    return a + b


def sigmoid(x):
    _gpu(x, "sigmoid")
    if _native16(x) and x.is_contiguous():
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _cabi.sigmoid_f16(x, out)
        return out
    return x.sigmoid()


def gather_rows(src, idx):
    """src [B,S,C], idx [B,K] int64 -> [B,K,C] = torch.gather(src, 1, idx[..., None].expand(-1, -1, C))"""
    _gpu(src, "gather_rows")
    C = src.shape[-1]
    if (_native16(src) and src.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous() and C % 4 == 0
            and src.data_ptr() % 16 == 0):
        out = torch.empty((idx.shape[0], idx.shape[1], C), dtype=src.dtype, device=src.device)
        with torch.cuda.device(src.device):
            _cabi.gather_rows(src, idx, out)
        return out
    return torch.gather(src, 1, idx.unsqueeze(-1).expand(-1, -1, C))


def decode_boxes_supported(coords_unact, idx):
    return _native16(coords_unact) and coords_unact.is_contiguous() and coords_unact.shape[-1] == 4 and idx.is_contiguous()


def decode_boxes(coords_unact, idx, num_classes, img_w, img_h):
    """head decode in one launch (reference co_dino_head.py:177-209): coords_unact [B,Nq,4] (box branch + reference,
    before the sigmoid), idx [B,K] into the flattened (query, class) scores -> (boxes [B,K,4] xyxy pixels, labels [B,K])"""
    _gpu(coords_unact, "decode_boxes")
    B, K = idx.shape
    boxes = torch.empty((B, K, 4), dtype=coords_unact.dtype, device=coords_unact.device)
    labels = torch.empty((B, K), dtype=torch.int64, device=coords_unact.device)
    with torch.cuda.device(coords_unact.device):
        _cabi.decode_boxes(coords_unact, idx, num_classes, img_w, img_h, boxes, labels)
    return boxes, labels


def valid_ratios(counts, level_wh):
    """counts [B,L,2] fp32 (mask_pyramid) , level_wh [L,2] (W_l, H_l) in the model dtype -> valid ratios [B,L,2]"""
    _gpu(counts, "valid_ratios")
    if _native16(level_wh) and counts.dtype == torch.float32 and counts.is_contiguous() and level_wh.is_contiguous():
        out = torch.empty(counts.shape, dtype=level_wh.dtype, device=counts.device)
        out32 = torch.empty(counts.shape, dtype=torch.float32, device=counts.device)
        with torch.cuda.device(counts.device):
            _cabi.valid_ratios(counts, level_wh, out, out32)
        if out32 is not None:
            out._codetr_f32 = out32   # counts / size unrounded: what the fp32 reference computes (query_sine_embed)
        return out
    return counts.to(level_wh.dtype) / level_wh
