#!/usr/bin/env python3
"""hip_ops.undistort_frames alone (csrc/undistort.hip), timed with HIP events on its launch stream, beside
hip_ops.orient_frames o = 3 on the same frames: that launch moves the same bytes (3 read and 3 written per pixel) without
computing anything, so it is the floor.  Three calibrations: a mild `brown` and a mild `fisheye` one, whose tiles all take
the staged path, and a zoom-out (fx' = fx / 3), whose tiles take the direct one; the share of direct tiles is computed
from the restatement tests/undistort_ref.py, which is also timed on one frame on the host.  The operators are timed in
turn, --rounds times over, each round --iters launches between one pair of events after a warm-up by time; the median
round and the spread are printed, one JSON line per operator.
    python tools/bench_undistort.py [--frames 8] [--size 1080 1920] [--rounds 7] [--iters 200]"""
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
TW, TH, BUDGET = 64, 16, 4864   # the kernel's tile and LDS window budget (csrc/undistort.hip)


def direct_share(ref, s, H, W):
    """the share of an image's sampling tiles whose source window is over the LDS budget"""
    X, Y, valid = ref.positions(s["params"], s["model"], *s["size"])
    xi, yi = X >> 5, Y >> 5
    live = valid & (xi >= -1) & (xi < W) & (yi >= -1) & (yi < H)
    over = tiles = 0
    for ty in range(0, s["size"][0], TH):
        for tx in range(0, s["size"][1], TW):
            m = live[ty:ty + TH, tx:tx + TW]
            if m.any():
                x, y = xi[ty:ty + TH, tx:tx + TW][m], yi[ty:ty + TH, tx:tx + TW][m]
                tiles += 1
                over += int(((x.max() - x.min() + 2) | 1) * (y.max() - y.min() + 2) > BUDGET)
    return over / max(tiles, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_undistort: no GPU; a timing needs one")
    import undistort_ref as ref
    from codetr import hip_ops

    dev = torch.device("cuda:0")
    (H, W), N = args.size, args.frames
    stride = -(-H * W * 3 // 16) * 16
    src = torch.randint(0, 256, (N * stride,), dtype=torch.uint8, device=dev)
    out = torch.empty_like(src)
    f = 0.6 * W
    cam = (f, f, 0.5 * W + 3.3, 0.5 * H - 2.1)
    calibrations = {
        "brown mild": dict(model="brown", camera_matrix=cam, dist_coeffs=(-0.25, 0.08, 0.001, -0.0005, -0.01)),
        "fisheye mild": dict(model="fisheye", camera_matrix=cam, dist_coeffs=(-0.02, 0.004, -0.001, 0.0002),
                             new_camera_matrix=(0.8 * f, 0.8 * f, cam[2], cam[3])),
        "brown zoom-out": dict(model="brown", camera_matrix=cam, dist_coeffs=(-0.25, 0.08, 0.001, -0.0005, -0.01),
                               new_camera_matrix=(f / 3, f / 3, cam[2], cam[3])),
    }
    settings = {k: hip_ops.undistort_settings(c, H, W) for k, c in calibrations.items()}
    rows = [(H, W, n * stride, 3 * W) for n in range(N)]
    ops = {"orient_frames o=3": lambda: hip_ops.orient_frames(src, [(3,) + r for r in rows], out)}
    for name, s in settings.items():
        ops["undistort_frames " + name] = lambda s=s: hip_ops.undistort_frames(src, rows, s, out)
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
    frame = src[:H * W * 3].cpu().numpy().reshape(H, W, 3)
    for name, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        line = dict(op=name, frames=N, H=H, W=W, us_median=round(med, 2), us_min=round(t[0], 2), us_max=round(t[-1], 2),
                    gb_per_s=round(moved / med / 1e3, 1), rounds=args.rounds, iters=args.iters)
        s = settings.get(name[len("undistort_frames "):])
        if s is not None:
            t0 = time.time()
            want = ref.remap(frame, s)
            line["numpy_ms_per_frame"] = round((time.time() - t0) * 1e3, 1)
            line["direct_tile_share"] = round(direct_share(ref, s, H, W), 4)
            got, _ = hip_ops.undistort_frames(src, rows[:1], s)
            line["equals_numpy"] = bool(np.array_equal(got[:H * W * 3].cpu().numpy().reshape(H, W, 3), want))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
