#!/usr/bin/env python3
"""hip_ops.orient_frames alone (csrc/orient.hip), timed with HIP events on its launch stream, beside
hip_ops.frames_to_rgb RGB -> RGB on the same frames: that launch moves the same bytes (3 read and 3 written per pixel)
without turning anything, so the ratio says what the mirrored reads (o = 3) and the pass through LDS (o = 6) cost.
The three are timed in turn, --rounds times over, each round --iters launches between one pair of events after a warm-up
by time; the median round and the spread are printed, one JSON line per operator.
    python tools/bench_orient.py [--frames 8] [--size 1080 1920] [--rounds 7] [--iters 200]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "co-detr-tensorrt_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_orient: no GPU; a timing needs one")
    from codetr import hip_ops

    dev = torch.device("cuda:0")
    (H, W), N = args.size, args.frames
    stride = -(-H * W * 3 // 16) * 16
    src = torch.randint(0, 256, (N * stride,), dtype=torch.uint8, device=dev)
    out = torch.empty_like(src)
    ops = {
        "frames_to_rgb rgb->rgb": lambda: hip_ops.frames_to_rgb(
            src, [("rgb", H, W, n * stride, 3 * W, 0, 0, 0, 0, n * stride) for n in range(N)], src.numel(), out=out),
        "orient_frames o=3": lambda: hip_ops.orient_frames(src, [(3, H, W, n * stride, 3 * W) for n in range(N)], out),
        "orient_frames o=6": lambda: hip_ops.orient_frames(src, [(6, H, W, n * stride, 3 * W) for n in range(N)], out),
    }
    times = {name: [] for name in ops}
    for name, op in ops.items():          # warm-up by time: code objects, clocks
        t0 = time.time()
        while time.time() - t0 < 0.5:
            op()
        torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, op in ops.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                op()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
    moved = 2 * N * H * W * 3
    for name, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        print(json.dumps(dict(op=name, frames=N, H=H, W=W, us_median=round(med, 2), us_min=round(t[0], 2), us_max=round(t[-1], 2),
                              gb_per_s=round(moved / med / 1e3, 1), rounds=args.rounds, iters=args.iters)))


if __name__ == "__main__":
    main()
