#!/usr/bin/env python3
"""hip_ops.enhance_frames alone (csrc/enhance.hip, two launches per call), timed with HIP events on its launch stream,
beside hip_ops.orient_frames o = 3 on the same bytes: that launch reads and writes the buffer once and computes nothing,
so it is the floor of the apply pass.  Three inputs: random bytes at grid 8 x 8 and at grid 1 x 1 (clip 2.0), and a
constant-colour frame at 8 x 8, where every lane of the histogram pass meets in one bin.  The operators are timed in turn,
--rounds times over, each round --iters calls between one pair of events after a warm-up by time; the median round and the
spread are printed, one JSON line per operator, with the restatement tests/enhance_ref.py timed on one frame on the host.
The two kernels apart: run this script under `rocprofv3 --kernel-trace --stats -- python tools/bench_enhance.py --rounds 1`
and read enhance_hist_kernel / enhance_apply_kernel off its kernel statistics.
    python tools/bench_enhance.py [--frames 8] [--size 1080 1920] [--rounds 7] [--iters 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "co-detr-tensorrt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_enhance: no GPU; a timing needs one")
    import enhance_ref as ref
    from codetr import hip_ops

    dev = torch.device("cuda:0")
    (H, W), N = args.size, args.frames
    stride = -(-H * W * 3 // 16) * 16
    random = torch.randint(0, 256, (N * stride,), dtype=torch.uint8, device=dev)
    constant = torch.tensor([200, 30, 90], dtype=torch.uint8, device=dev).repeat(N * stride // 3 + 1)[:N * stride].contiguous()
    out, cache = torch.empty_like(random), {}
    rows = [(H, W, n * stride, 3 * W) for n in range(N)]
    cases = {"random 8x8": (random, dict(grid=(8, 8), clip_limit=2.0)), "random 1x1": (random, dict(grid=(1, 1), clip_limit=2.0)),
             "constant 8x8": (constant, dict(grid=(8, 8), clip_limit=2.0))}
    ops = {"orient_frames o=3": lambda: hip_ops.orient_frames(random, [(3,) + r for r in rows], out)}
    for name, (src, s) in cases.items():
        ops["enhance_frames " + name] = lambda src=src, s=s: hip_ops.enhance_frames(src, rows, s, out, workspace=cache)
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
    for name, t in times.items():
        t = sorted(t)
        line = dict(op=name, frames=N, H=H, W=W, us_median=round(t[len(t) // 2], 2), us_min=round(t[0], 2), us_max=round(t[-1], 2),
                    rounds=args.rounds, iters=args.iters)
        case = cases.get(name[len("enhance_frames "):])
        if case is not None:
            src, s = case
            frame = src[:H * W * 3].cpu().numpy().reshape(H, W, 3)
            t0 = time.time()
            want = ref.enhance(frame, **s)
            line["numpy_ms_per_frame"] = round((time.time() - t0) * 1e3, 1)
            got, _ = hip_ops.enhance_frames(src, rows[:1], s)
            line["equals_numpy"] = bool(np.array_equal(got[:H * W * 3].cpu().numpy().reshape(H, W, 3), want))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
