#!/usr/bin/env python3
"""Co-DINO R50 (BASELINE config 1's model) in 16 bits: ms per image of the whole forward, and of the backbone alone, for
the three backbone routes --
  native  ResNet.forward_tokens on libcodetr_hip.so (implicit-GEMM 3x3 / strided 1x1 convs, BN folded)
  im2col  the same with the 3x3 / strided convs as codetr_im2col_tokens_b16 + codetr_linear_* (hip_ops.R50_CONV_IM2COL)
  miopen  the NCHW route (hip_ops.R50_NATIVE = False): MIOpen convolutions + ATen BN / ReLU / add / max pool
at 608x608 (config 1's size) and 1333x800 (the config's test scale), batch 1 and 4, fp16 and bf16.  Random weights of
the real architecture (init_weights), frozen-BN statistics drawn once.  One JSON line per (dtype, size, batch, route).
    python tools/bench_r50.py [--steps 10] [--warmup 3] [--dtypes fp16,bf16] [--sizes 608x608,1333x800] [--batches 1,4]
        [--routes native,im2col,miopen]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "co-detr-tensorrt_amd"))
CFG = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs", "co_dino_5scale_r50_8xb2_1x_coco.py")
ROUTES = {"native": dict(R50_NATIVE=True, R50_CONV_IM2COL=False), "im2col": dict(R50_NATIVE=True, R50_CONV_IM2COL=True),
          "miopen": dict(R50_NATIVE=False, R50_CONV_IM2COL=False)}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--sizes", default="608x608,1333x800", help="WxH list")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--routes", default="native,im2col,miopen")
    a = ap.parse_args()
    import codetr
    from codetr import hip_ops

    torch.manual_seed(0)
    base = codetr.build_CoDETR(CFG, None, "cpu")
    base.init_weights()
    g = torch.Generator().manual_seed(1)
    for name, buf in base.named_buffers():
        if name.endswith("running_var"):
            buf.copy_(torch.rand(buf.shape, generator=g) + 0.5)
        elif name.endswith("running_mean"):
            buf.copy_(torch.randn(buf.shape, generator=g) * 0.1)
    dev = torch.device("cuda")
    for dname in a.dtypes.split(","):
        dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[dname]
        model = base.to(dev).to(dtype).eval()
        for size in a.sizes.split(","):
            W, H = (int(t) for t in size.split("x"))
            for B in (int(t) for t in a.batches.split(",")):
                gi = torch.Generator(device=dev).manual_seed(B * H + W)
                img = torch.randn(B, 3, H, W, device=dev, generator=gi).to(dtype)
                mask = torch.zeros(B, H, W, device=dev, dtype=dtype)
                for route in a.routes.split(","):
                    sw = ROUTES[route]
                    for k, v in sw.items():
                        setattr(hip_ops, k, v)
                    try:
                        with torch.no_grad():
                            cap = {}
                            model(img, mask, capture=cap)
                            if route == "miopen":
                                bb = lambda: model.backbone(img)  # noqa: E731
                            else:
                                bb = lambda: model.backbone.forward_tokens(img)  # noqa: E731
                            ms = timed(lambda: model(img, mask), a.steps, a.warmup)
                            ms_bb = timed(bb, a.steps, a.warmup)
                    finally:
                        for k, v in ROUTES["native"].items():
                            setattr(hip_ops, k, v)
                    print(json.dumps({"dtype": dname, "size": f"{W}x{H}", "batch": B, "route": route,
                                      "model_route": cap["route"], "ms_per_image": round(ms / B, 3),
                                      "backbone_ms_per_image": round(ms_bb / B, 3)}), flush=True)
        base = model


if __name__ == "__main__":
    main()
