#!/usr/bin/env python3
"""hip_ops.raw_to_rgb alone (csrc/raw.hip), timed with HIP events on its launch stream -- 8-bit and 12-bit frames, Malvar
and bilinear -- beside hip_ops.frames_to_rgb GRAY -> RGB on the same 8-bit frames (the kernel that moves the same 1 + 3
bytes per pixel with no stencil) and a device-to-device copy that reads and writes as many bytes together.  The operators
are timed in turn, --rounds times over, each round --iters launches between one pair of events after a warm-up by time;
the median round and the spread are printed, one JSON line per operator.
With --inferencer also images/s of the Inferencer (fp16, Swin-L config, random weights) at batch_size 8 over --images
frames of the same size, three ways in turn: fed as bayer_rggb mosaics from the host; fed as RGB arrays demosaiced
beforehand (that conversion not timed); and with the numpy restatement (tests/raw_ref.py) demosaicing on the host inside
the timed pass -- the route the stage replaces.
    python tools/bench_raw.py [--frames 8] [--size 1080 1920] [--rounds 7] [--iters 200] [--inferencer] [--images 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "co-detr-tensorrt_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT):
    sys.path.insert(0, _p)


def operators(args):
    from codetr import hip_ops

    dev = torch.device("cuda:0")
    (H, W), N = args.size, args.frames
    stride = -(-H * W * 3 // 16) * 16
    src8 = torch.randint(0, 256, (N * H * W,), dtype=torch.uint8, device=dev)
    src12 = torch.randint(0, 4096, (N * H * W,), dtype=torch.int16, device=dev).view(torch.uint8)
    out = torch.empty((N * stride,), dtype=torch.uint8, device=dev)
    a, b = torch.empty((N * H * W * 2,), dtype=torch.uint8, device=dev), torch.empty((N * H * W * 2,), dtype=torch.uint8, device=dev)
    ops = {"frames_to_rgb gray->rgb": (4, lambda: hip_ops.frames_to_rgb(
        src8, [("gray", H, W, n * H * W, W, 0, 0, 0, 0, n * stride) for n in range(N)], out.numel(), out=out)),
        "copy of (1+3)/2 bytes per pixel": (4, lambda: b.copy_(a))}
    for bits, src in ((8, src8), (12, src12)):
        B = 1 if bits == 8 else 2
        rows = [("bayer_rggb", bits, H, W, n * H * W * B, W * B, n * stride) for n in range(N)]
        for method in ("malvar", "bilinear"):
            s = hip_ops.raw_settings(dict(bits=bits, method=method))
            ops[f"raw_to_rgb {bits}-bit {method}"] = (B + 3, lambda src=src, rows=rows, s=s: hip_ops.raw_to_rgb(src, rows, out.numel(), s, out=out))
    times = {name: [] for name in ops}
    for name, (_, op) in ops.items():          # warm-up by time: code objects, clocks
        t0 = time.time()
        while time.time() - t0 < 0.5:
            op()
        torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (_, op) in ops.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                op()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
    for name, t in times.items():
        t = sorted(t)
        med, moved = t[len(t) // 2], ops[name][0] * N * H * W
        print(json.dumps(dict(op=name, frames=N, H=H, W=W, us_median=round(med, 2), us_min=round(t[0], 2), us_max=round(t[-1], 2),
                              bytes_moved=moved, gb_per_s=round(moved / med / 1e3, 1), rounds=args.rounds, iters=args.iters)), flush=True)


def inferencer(args):
    import bench_inferencer
    import raw_ref

    inf = bench_inferencer.inferencers()["fp16"]
    (H, W), rng = args.size, np.random.default_rng(3)
    yy, xx = np.mgrid[:H, :W]
    base = ((xx * 255 // (W - 1) + yy * 255 // (H - 1)) // 2).astype(np.int16)
    mosaics = [np.clip(base + rng.integers(-6, 7, base.shape, dtype=np.int16), 0, 255).astype(np.uint8) for _ in range(args.images)]
    t0 = time.perf_counter()
    rgb = [np.ascontiguousarray(raw_ref.demosaic(m, "bayer_rggb")) for m in mosaics]
    host_ms = (time.perf_counter() - t0) / len(mosaics) * 1e3
    kw = dict(device="cuda:0", dtype=torch.float16, batch_size=8)
    arms = {"bayer_rggb_from_host": lambda: inf(mosaics, input_format="bayer_rggb", **kw),
            "rgb_demosaiced_beforehand": lambda: inf(rgb, **kw),
            "numpy_demosaic_inside_the_pass": lambda: inf([np.ascontiguousarray(raw_ref.demosaic(m, "bayer_rggb")) for m in mosaics], **kw)}
    same = arms["bayer_rggb_from_host"]()["predictions"] == arms["rgb_demosaiced_beforehand"]()["predictions"]
    passes = {name: [] for name in arms}
    with torch.no_grad():
        for _ in range(args.repeats):
            for name, call in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                passes[name].append(round(time.perf_counter() - t0, 4))
    print(json.dumps(dict(inferencer="fp16 batch_size 8", images=args.images, H=H, W=W, same_predictions=bool(same),
                          numpy_demosaic_ms_per_frame=round(host_ms, 1),
                          **{name: dict(images_per_s=round(args.images / min(t), 2), pass_s=t) for name, t in passes.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--inferencer", action="store_true")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raw: no GPU; a timing needs one")
    operators(args)
    if args.inferencer:
        inferencer(args)


if __name__ == "__main__":
    main()
