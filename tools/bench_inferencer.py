"""Images/s of the user-facing `codetr.Inferencer` (image in, detections out) at batch_size 1, 4 and 8, fp16 and bf16.

Swin-L config (Resize + Pad to 1152x768), seeded random weights (bench.build_model), 32 synthetic RGB uint8 images of
mixed sizes (640x480, 1280x720, 1920x1080, 800x1333, cycled).  A timed pass is `inf(images, batch_size=B)` over all 32
images and ends with their detections on the host as Python lists, so the host clock around it is the user's latency;
each figure is the best of --repeats passes after one warm-up pass.  fp16 at batch_size 1 is the per-image path
(preprocess_image, F.pad, batched_nms, per-image syncs); every other cell is the batched path (one upload, one
preprocess_batch launch, one forward, one postprocess_detections launch, one download per chunk).  The `fp16_soft_nms`
row is the same fp16 model behind `Inferencer(..., nms_type="config")`: soft-NMS + max_per_img as the config asks, the
batched path at every batch size with one postprocess_softnms launch per chunk.

`postprocess_launch_us`: the two post-processing kernels alone on the same inputs -- 8 images x 300 candidates, fp16,
no score threshold (every candidate live), IoU 0.8, labels random over 80 classes / all candidates under one label --
HIP events around 200 back-to-back launches after 20 warm-up launches, microseconds per launch.

Kernel times: unless --no-profile, a child process runs the same Inferencer calls (batch 8 over 16 images in fp16 and
bf16, batch 1 over 4 images in fp16) under `rocprofv3 --kernel-trace --stats`; the per-launch times of the pre- and
post-processing kernels are read from its kernel statistics.

`--tta` adds a `tta` sub-record (test-time augmentation, fp16): images/s of `Inferencer(tta=dict(scales=TTA_SCALES,
flip=...))` at batch_size 4 over --tta-images images, with and without the flip, beside the sum of three plain runs of
the same Inferencer with its Resize set to each scale (and no fixed Pad) -- the way to the same unflipped views without
the feature --, and with the flip merged by weighted boxes fusion (`wbf=dict()`) instead of NMS; and the TTA kernels
alone, HIP events as above: tta_merge and wbf_merge at N = 8, Q = 300 with 2 and 6 views for both label layouts,
preprocess_views beside preprocess_batch on the same 8 images resized into (1152, 768) (twice the rows: each
image plain and mirrored).

`--vis` adds a `vis` sub-record (the visualisation, fp16): images/s of `Inferencer(visualizer={})` at batch_size 8 with
`return_vis` on (pred_score_thr 0: every detection is drawn) and off; draw_detections_kernel alone, HIP events as above,
on 8 images of 1920x1280 with 300 and with 20 drawn detections each; and the device-to-host copy of that buffer, the
one extra transfer a visualising chunk makes.

`--vis png` / `--vis jpeg` print only a `vis_files` record (fp16): images/s of `Inferencer(visualizer={},
vis_format=...)(frames, out_dir=<a tmpfs directory>)` at batch_size 8 over --images 1920x1080 frames (a gradient with +-6
of noise), alternating with the same call of an Inferencer without a visualiser; with `jpeg` also the two encoder
launches alone on eight of the frames (HIP events, bytes read + written per second beside a device-to-device copy of as
many bytes) and Pillow's host encoder on one frame.

`--slice` adds a `slice` sub-record (sliced inference, fp16): images/s of `Inferencer(slicing=dict(tile=(1280, 1280),
overlap=0.2, full_image=True))` at batch_size 2 over --slice-images synthetic 3840x2160 images (8 tiles + the image: 9
views each), beside the host composition it replaces on the same images -- per image the tiles cropped on the host, one
plain `Inferencer` call over the image's 9 crops at batch_size = tile_batch (no fixed Pad step, as the sliced path), the
detections shifted and fused in numpy (tests/slice_ref.py) --; and the two slicing kernels alone, HIP events as above:
preprocess_tiles on the 9 rows of one such image, slice_merge at N = 2, V = 9, Q = 300 for both merge types.

`--frames nv12|i420|bgr [--resident]` prints only a `frames` record (decoder frames, fp16): frames_to_rgb_kernel alone
on eight 1920x1080 frames of the format -- a HIP event pair around each of 200 launches, the median in microseconds
and the achieved GB/s of (bytes read + bytes written) beside a torch device-to-device copy of the same byte count in the same run --; and images/s of
the Inferencer at batch_size 8 over --images frames of 1920x1080 fed as host frames of the format, (with --resident)
as GPU-resident tensors, and as host RGB arrays converted beforehand (the conversion is not timed: the fairest thing
the RGB-only route can do), the three in turn, three times.

`--track` prints only a `track` record (tracking, fp16; the greedy and the optimal association alternating, a crowd of
overlapping objects with the solver's rounds per frame, codetr_assign_i32 beside scipy, and a tracked-optimal arm of the
Inferencer): the tracking kernels alone on 300 detection rows of which 100 are
moving objects -- HIP event pairs as above, 8 frames of one stream in a launch and one frame of each of 8 streams --;
and images/s of the Inferencer at batch_size 8 over --images images taken as the frames of one stream with
`tracker={}`, without a tracker, and with the host composition the tracker replaces (the untracked call's predictions
through tests/track_ref.py frame by frame, the state on the host), the three in turn, three times.

`--track --motion` prints only a `track_motion` record (camera-motion compensation, fp16): estimate_motion's three
launches alone on 8 frames of 1920x1080 beside a device-to-device copy of the same bytes (HIP event pairs, median of 200);
track_update on the two `--track` workloads with and without a motion operand, alternating; and images/s of the tracked
Inferencer at batch_size 8 over 16 panned 1920x1080 frames as one stream, with and without `track_motion`, in turn.
`--track --motion similarity` adds the similarity model beside each of them: the estimate's five launches (their excess
over the three is the fit), the same on 8 frames of 320x320 with all 81 blocks textured, track_update with [N, 8] rows,
and the Inferencer with `track_motion="similarity"`.

`--track --appearance` prints only a `track_appearance` record (the appearance cue, fp16): appearance_descriptors alone at
N = 8, Q = 300 on 1920x1080 frames beside a device-to-device copy of the bytes it samples (HIP event pairs, median of 200);
track_update on the two `--track` workloads with and without the descriptors, greedy and optimal, alternating; and images/s
of the tracked Inferencer at batch_size 8 over 16 frames of 1920x1080 as one stream, with and without `track_appearance`.

`--decode jpeg` prints only a `decode` record (JPEG files as input, fp16): --images frames of 1920x1080 (the gradient
with noise of `--vis`) written as 4:2:0 files by Pillow where it imports (no restart markers), else by encode_jpeg; the
decoder's five launches alone on eight of them (HIP event pairs, median), the bytes uploaded beside the bytes written,
the host parser per file, Pillow's decode per frame; and images/s of the Inferencer at batch_size 8 fed the files
(`input_format="jpeg"`), the same files decoded by Pillow inside the timed pass, and arrays decoded beforehand, in turn.

`--redact MODE` prints only a `redact` record (redaction of detected regions, fp16; MODE is pixelate, blur or fill):
redact_detections alone per mode on 8 frames of 1920x1080 at N = 8, Q = 300 with 20 person-sized boxes per frame (HIP event
pairs, median of 200), beside a device-to-device copy of the buffer's bytes, draw_detections on the same operands, the
same frames with no selected row (the early exit) and the numpy restatement on one frame; and images/s of
`Inferencer(visualizer={}, vis_format="jpeg")(frames, out_dir=...)` at batch_size 8 with and without `redact=dict(mode=MODE)`,
alternating.

    python tools/bench_inferencer.py [--images 32] [--repeats 3] [--no-profile] [--tta] [--vis] [--slice]   -> one JSON line
    python tools/bench_inferencer.py --frames nv12 --resident
    python tools/bench_inferencer.py --track
    python tools/bench_inferencer.py --track --motion
    python tools/bench_inferencer.py --track --motion similarity
    python tools/bench_inferencer.py --track --appearance
    python tools/bench_inferencer.py --redact blur
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "co-detr-tensorrt_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
SIZES_WH = [(640, 480), (1280, 720), (1920, 1080), (800, 1333)]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
KERNELS = ("preprocess_batch_kernel", "postprocess_softnms_kernel", "postprocess_kernel", "preprocess_kernel",
           "batched_nms_kernel")


def synthetic_images(n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (SIZES_WH[i % 4][1], SIZES_WH[i % 4][0], 3), dtype=np.uint8) for i in range(n)]


def inferencers():
    """one Inferencer per dtype over copies of one seeded random-init Swin-L model"""
    import copy

    import bench
    import codetr
    from codetr.inferencer import Inferencer

    torch.manual_seed(42)
    base = codetr.build_CoDETR(bench.CFG, None, "cpu")
    base.init_weights()
    bench.set_offset_noise(base, 2.0, 42)
    out = {}
    for name, dt in DTYPES.items():
        model = copy.deepcopy(base).to(device=DEV, dtype=dt).eval()
        out[name] = Inferencer(model, bench.CFG, dataset_meta=None)
    return out


def post_kernel_times(launches=200, warmup=20):
    """us per launch of postprocess_softnms_kernel and postprocess_kernel on the same 8 x 300 fp16 candidates"""
    from codetr import hip_ops

    g = torch.Generator().manual_seed(0)
    N, Q = 8, 300
    c = torch.rand(N, Q, 2, generator=g) * 800
    wh = torch.rand(N, Q, 2, generator=g) * 150 + 2
    boxes = torch.cat((c, c + wh), -1)
    boxes[:, Q // 2:] = boxes[:, :Q - Q // 2] + (torch.rand(N, Q - Q // 2, 4, generator=g) - 0.5) * 6   # near duplicates
    boxes, scores = boxes.half().to(DEV), torch.rand(N, Q, generator=g).half().to(DEV)
    div = torch.full((N, 4), 0.6, dtype=torch.float16, device=DEV)
    out = {}
    for name, labels in (("80_classes", torch.randint(0, 80, (N, Q), generator=g)), ("one_label", torch.zeros(N, Q).long())):
        labels = labels.to(DEV)
        calls = {"postprocess_softnms_kernel": lambda: hip_ops.postprocess_detections_soft(boxes, scores, labels, div, None, 0.8,
                                                                                          "linear", 1e-3, 300),
                 "postprocess_kernel": lambda: hip_ops.postprocess_detections(boxes, scores, labels, div, None, 0.8)}
        out[name] = {}
        for kernel, call in calls.items():
            for _ in range(warmup):
                dets = call()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(launches):
                dets = call()
            t1.record()
            torch.cuda.synchronize()
            out[name][kernel] = {"us_per_launch": round(t0.elapsed_time(t1) * 1e3 / launches, 2),
                                 "detections": int(dets.count.sum())}
    return out


TTA_SCALES = [(960, 640), (1152, 768), (1344, 896)]


def _event_us(call, launches=200, warmup=20):
    for _ in range(warmup):
        call()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(launches):
        call()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) * 1e3 / launches, 2)


def tta_kernel_times():
    """us per launch of tta_merge_kernel (N = 8, Q = 300, fp16; V = 2 and 6; hard NMS at 0.5 and linear soft-NMS), of
    wbf_merge_kernel on the same inputs (conf_type avg, IoU 0.55) and of preprocess_views_kernel beside
    preprocess_batch_kernel"""
    from codetr import hip_ops
    from codetr.inferencer import rescale_size

    g = torch.Generator().manual_seed(0)
    N, Q = 8, 300
    c = torch.rand(N, Q, 2, generator=g) * 800
    wh = torch.rand(N, Q, 2, generator=g) * 150 + 2
    base = torch.cat((c, c + wh), -1)
    widths = torch.full((N,), 1000.0, device=DEV)
    out = {"tta_merge_kernel": {}, "wbf_merge_kernel": {}}
    for V in (2, 6):
        boxes = (base[None] + (torch.rand(V, N, Q, 4, generator=g) - 0.5) * 6).half().to(DEV)   # near duplicates across views
        scores = torch.rand(V, N, Q, generator=g).half().to(DEV)
        count = torch.full((V * N,), Q, dtype=torch.int32, device=DEV)
        for name, labels in (("80_classes", torch.randint(0, 80, (N, Q), generator=g)), ("one_label", torch.zeros(N, Q).long())):
            labels = labels[None].expand(V, N, Q).contiguous().to(DEV)
            dets = [hip_ops.Detections(boxes.view(V * N, Q, 4), scores.view(V * N, Q), labels.view(V * N, Q), count, None)]
            for mode, nms in (("hard", dict(type="nms", iou_threshold=0.5)),
                              ("soft_linear", dict(type="soft_nms", iou_threshold=0.5, method="linear"))):
                call = lambda: hip_ops.tta_merge(dets, [v % 2 == 1 for v in range(V)], widths, nms, 300)  # noqa: E731
                out["tta_merge_kernel"][f"V{V}_{name}_{mode}"] = {"us_per_launch": _event_us(call),
                                                                  "detections": int(call().count.sum())}
            call = lambda: hip_ops.wbf_merge(dets, [v % 2 == 1 for v in range(V)], widths, None, 300)  # noqa: E731
            out["wbf_merge_kernel"][f"V{V}_{name}"] = {"us_per_launch": _event_us(call), "detections": int(call().count.sum())}
    images = synthetic_images(N, seed=2)
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    rows, off = [], 0
    for im in images:
        nh, nw = rescale_size(im.shape[0], im.shape[1], (1152, 768))
        rows.append((off, im.shape[0], im.shape[1], nh, nw, nh, nw))
        off += im.size
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    rows8 = [r + (f,) for f in (0, 1) for r in rows]
    out["preprocess_batch_kernel_8_rows_us"] = _event_us(
        lambda: hip_ops.preprocess_batch(src, rows, (1152, 1152), mean, std, dtype=torch.float16))
    out["preprocess_views_kernel_8_plain_rows_us"] = _event_us(
        lambda: hip_ops.preprocess_views(src, rows8[:8], (1152, 1152), mean, std, dtype=torch.float16))
    out["preprocess_views_kernel_16_rows_us"] = _event_us(
        lambda: hip_ops.preprocess_views(src, rows8, (1152, 1152), mean, std, dtype=torch.float16))
    return out


def _passes(inf, images, bs, repeats):
    """seconds of every timed pass of inf(images, batch_size=bs) after one warm-up pass"""
    with torch.no_grad():
        inf(images[:bs], device=DEV, dtype=torch.float16, batch_size=bs)
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf(images, device=DEV, dtype=torch.float16, batch_size=bs)
            times.append(time.perf_counter() - t0)
    return times


def tta_record(inf, n_images, repeats, bs=4):
    import bench
    from codetr.inferencer import Inferencer

    images = synthetic_images(n_images, seed=3)
    rec = {"scales": TTA_SCALES, "batch_size": bs, "images": n_images, "repeats": repeats, "dtype": "fp16"}
    for name, flip, merge in (("tta_3_scales_flip", True, dict(nms=dict(type="nms", iou_threshold=0.6))),
                              ("tta_3_scales", False, dict(nms=dict(type="nms", iou_threshold=0.6))),
                              ("tta_3_scales_flip_wbf", True, dict(wbf=dict()))):
        t = Inferencer(inf.model, bench.CFG, dataset_meta=None, tta=dict(scales=TTA_SCALES, flip=flip, max_per_img=100, **merge))
        times = _passes(t, images, bs, repeats)
        rec[name] = {"images_per_s": round(n_images / min(times), 3), "pass_s": [round(v, 4) for v in times]}
    # the Inferencer reads `scale` and `pad_size` on every call (preprocess_batch), so one instance serves all scales
    plain, total = Inferencer(inf.model, bench.CFG, dataset_meta=None), []
    plain.pad_size = None
    for scale in TTA_SCALES:
        plain.scale = scale
        total.append(_passes(plain, images, bs, repeats))
    sums = [sum(t[i] for t in total) for i in range(repeats)]
    rec["three_plain_runs"] = {"images_per_s": round(n_images / sum(min(t) for t in total), 3),
                               "pass_s_per_scale": [[round(v, 4) for v in t] for t in total], "sum_s": [round(v, 4) for v in sums]}
    rec["kernels_us"] = tta_kernel_times()
    return rec


SLICE = dict(tile=(1280, 1280), overlap=0.2, full_image=True, tile_batch=8, max_per_img=300)
SLICE_WH = (3840, 2160)


def slice_kernel_times(image):
    """us per launch of preprocess_tiles_kernel (the 9 rows of one 3840x2160 image into the (1152, 768) scale, fp16) and of
    slice_merge_kernel (N = 2, V = 9, Q = 300, fp16, 80 classes; nmm / ios and nms / iou at 0.5)"""
    from codetr import hip_ops
    from codetr.inferencer import Inferencer, rescale_size

    H, W = image.shape[:2]
    views = Inferencer.slice_grid(H, W, SLICE["tile"], SLICE["overlap"]) + [(0, 0, H, W)]
    rows = [(0, H, W, y, x, h, w) + rescale_size(h, w, (1152, 768)) * 2 for y, x, h, w in views]
    src = torch.from_numpy(image.reshape(-1)).to(DEV)
    hw = (max(r[7] for r in rows), max(r[8] for r in rows))
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    out = {"preprocess_tiles_kernel_9_rows_us": _event_us(
        lambda: hip_ops.preprocess_tiles(src, rows, hw, mean, std, dtype=torch.float16), launches=50, warmup=5),
        "preprocess_tiles_batch_hw": list(hw), "slice_merge_kernel": {}}
    g = torch.Generator().manual_seed(0)
    N, V, Q = 2, len(views), 300
    c = torch.rand(N, Q, 2, generator=g) * torch.tensor([W, H])
    wh = torch.rand(N, Q, 2, generator=g) * 300 + 8
    base = torch.cat((c - wh / 2, c + wh / 2), -1)
    origins = torch.tensor([[float(x), float(y)] for y, x, _, _ in views] * N)
    boxes = (base[:, None] + (torch.rand(N, V, Q, 4, generator=g) - 0.5) * 6).view(N * V, Q, 4) - origins.repeat(1, 2)[:, None]
    dets = hip_ops.Detections(boxes.half().to(DEV), torch.rand(N * V, Q, generator=g).half().to(DEV),
                              torch.randint(0, 80, (N, 1, Q), generator=g).expand(N, V, Q).reshape(N * V, Q).to(DEV),
                              torch.full((N * V,), Q, dtype=torch.int32, device=DEV), None)
    table = torch.arange(N * V, dtype=torch.int32, device=DEV).view(N, V)
    sizes = torch.tensor([[float(W), float(H)]] * N, device=DEV)
    origins = origins.to(DEV)
    for name, merge in (("nmm_ios", dict(type="nmm", metric="ios", threshold=0.5)),
                        ("nms_iou", dict(type="nms", metric="iou", threshold=0.5))):
        call = lambda: hip_ops.slice_merge(dets, table, origins, sizes, merge, 300)  # noqa: E731
        out["slice_merge_kernel"][name] = {"us_per_launch": _event_us(call), "detections": int(call().count.sum())}
    return out


def slice_record(inf, n_images, repeats, bs=2):
    import bench
    from codetr.inferencer import Inferencer

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import slice_ref

    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (SLICE_WH[1], SLICE_WH[0], 3), dtype=np.uint8) for _ in range(n_images)]
    rec = {"slicing": SLICE, "image_wh": SLICE_WH, "batch_size": bs, "images": n_images, "repeats": repeats, "dtype": "fp16"}
    sliced = Inferencer(inf.model, bench.CFG, dataset_meta=None, slicing=SLICE)
    times = _passes(sliced, images, bs, repeats)
    rec["views_per_image"] = len(sliced.slice_rows([0], [images[0].shape[:2]])[0])
    rec["sliced"] = {"images_per_s": round(n_images / min(times), 3), "pass_s": [round(v, 4) for v in times]}
    plain = Inferencer(inf.model, bench.CFG, dataset_meta=None)
    plain.pad_size = None
    merge = sliced.slicing["merge"]

    def composed(image):
        H, W = image.shape[:2]
        views = slice_ref.grid(H, W, SLICE["tile"], (SLICE["overlap"],) * 2) + [(0, 0, H, W)]
        crops = [np.ascontiguousarray(image[y:y + h, x:x + w]) for y, x, h, w in views]
        preds = plain(crops, device=DEV, dtype=torch.float16, batch_size=SLICE["tile_batch"])["predictions"]
        Q = max(1, max(len(p["labels"]) for p in preds))
        boxes, scores = np.zeros((len(views), Q, 4), np.float32), np.zeros((len(views), Q), np.float32)
        labels, count = np.zeros((len(views), Q), np.int64), np.zeros(len(views), np.int64)
        for r, p in enumerate(preds):
            n = count[r] = len(p["labels"])
            boxes[r, :n], scores[r, :n], labels[r, :n] = np.asarray(p["bboxes"]).reshape(n, 4), p["scores"], p["labels"]
        return slice_ref.merge(boxes, scores, labels, count, range(len(views)), [(x, y) for y, x, _, _ in views], (W, H),
                               metric=merge["metric"], mode=merge["type"], threshold=merge["threshold"],
                               class_agnostic=merge["class_agnostic"], max_keep=SLICE["max_per_img"])

    with torch.no_grad():
        composed(images[0])
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for image in images:
                composed(image)
            times.append(time.perf_counter() - t0)
    rec["host_composition"] = {"images_per_s": round(n_images / min(times), 3), "pass_s": [round(v, 4) for v in times]}
    rec["speedup"] = round(rec["sliced"]["images_per_s"] / rec["host_composition"]["images_per_s"], 3)
    rec["kernels_us"] = slice_kernel_times(images[0])
    return rec


def draw_kernel_times(N=8, H=1280, W=1920, Q=300):
    """us per launch of draw_detections_kernel on N images of W x H with Q and with 20 drawn detections each (fp16,
    default style, 80 classes), and the device-to-host copy of the buffer"""
    from codetr import hip_ops
    from codetr.inferencer import generated_palette

    g = torch.Generator().manual_seed(0)
    c = torch.rand(N, Q, 2, generator=g) * torch.tensor([W, H])
    wh = torch.rand(N, Q, 2, generator=g) * torch.tensor([W / 3, H / 3]) + 8
    boxes = torch.cat((c - wh / 2, c + wh / 2), -1).half().to(DEV)
    scores = (torch.rand(N, Q, generator=g) * 0.6 + 0.35).half().to(DEV)
    labels = torch.randint(0, 80, (N, Q), generator=g).to(DEV)
    buf = torch.randint(0, 256, (N * H * W * 3,), dtype=torch.uint8, generator=g).to(DEV)
    rows = [(n * H * W * 3, H, W) for n in range(N)]
    names = hip_ops.draw_names_table([f"class {i}" for i in range(80)]).to(DEV)
    colors = torch.tensor(generated_palette(80), dtype=torch.uint8, device=DEV)
    out = {"images": N, "image_wh": [W, H], "buffer_bytes": buf.numel()}
    for drawn in (Q, 20):
        dets = hip_ops.Detections(boxes, scores, labels, torch.full((N,), drawn, dtype=torch.int32, device=DEV), None)
        out[f"draw_detections_kernel_{drawn}_drawn_us"] = _event_us(
            lambda: hip_ops.draw_detections(buf, rows, dets, names, colors), launches=50, warmup=5)
    buf.cpu()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        buf.cpu()
        times.append(time.perf_counter() - t0)
    out["download_ms"] = round(min(times) * 1e3, 3)
    out["download_gb_per_s"] = round(buf.numel() / min(times) / 1e9, 2)
    return out


def vis_record(inf, images, repeats, bs=8):
    import bench
    from codetr.inferencer import Inferencer

    v = Inferencer(inf.model, bench.CFG, dataset_meta=None, visualizer={})
    rec = {"batch_size": bs, "images": len(images), "repeats": repeats, "dtype": "fp16", "pred_score_thr": 0.0}
    for name, on in (("return_vis_off", False), ("return_vis_on", True), ("return_vis_off_again", False),
                     ("return_vis_on_again", True)):
        with torch.no_grad():
            v(images[:bs], return_vis=on, pred_score_thr=0.0, device=DEV, dtype=torch.float16, batch_size=bs)
            times = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = v(images, return_vis=on, pred_score_thr=0.0, device=DEV, dtype=torch.float16, batch_size=bs)
                times.append(time.perf_counter() - t0)
        rec[name] = {"images_per_s": round(len(images) / min(times), 2), "pass_s": [round(t, 4) for t in times]}
    rec["detections_per_image"] = round(sum(len(p["labels"]) for p in out["predictions"]) / len(images), 1)
    rec["image_bytes_per_pass"] = int(sum(im.size for im in images))
    rec["kernels"] = draw_kernel_times()
    return rec


def vis_frames(n, seed=3):
    """n 1920x1080 RGB frames: a colour gradient with +-6 of noise per channel, a new noise field per frame (the entropy
    of a photograph; uniform noise, which synthetic_images makes, is the worst case of any image coder)"""
    rng = np.random.default_rng(seed)
    H, W = 1080, 1920
    yy, xx = np.mgrid[:H, :W]
    base = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (W + H - 2)], -1).astype(np.int16)
    return [np.clip(base + rng.integers(-6, 7, base.shape, dtype=np.int16), 0, 255).astype(np.uint8) for _ in range(n)]


def jpeg_kernel_times(frames, quality=90, subsampling="420"):
    """us per codetr_jpeg_encode_u8 call (both launches) on the frames, the bytes it has to read and write (the RGB
    images and the scans) per second, beside a device-to-device copy of as many bytes, and Pillow's host encoder on one of
    the frames where Pillow imports"""
    from codetr import _jpeg, hip_ops

    N, (H, W) = len(frames), frames[0].shape[:2]
    src = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(DEV)
    rows = [(n * H * W * 3, H, W) for n in range(N)]
    sub = _jpeg.SUBSAMPLINGS[subsampling]
    stride = hip_ops.jpeg_out_stride(rows, subsampling)
    out = torch.empty((N * stride,), dtype=torch.uint8, device=DEV)
    lengths = torch.empty((N,), dtype=torch.int32, device=DEV)
    ws = torch.empty((_jpeg.workspace_bytes(rows, sub, stride),), dtype=torch.uint8, device=DEV)
    _jpeg.encode(src, rows, quality, sub, out, stride, lengths, ws)
    scan = [int(v) for v in lengths.cpu()]
    moved = src.numel() + sum(scan)
    a, b = torch.randint(0, 256, (moved // 2,), dtype=torch.uint8).to(DEV), torch.empty((moved // 2,), dtype=torch.uint8,
                                                                                      device=DEV)
    rec = {"frames": N, "frame_wh": [W, H], "quality": quality, "subsampling": subsampling, "bytes_read": src.numel(),
           "bytes_written": sum(scan), "scan_bytes_per_frame": scan, "out_stride": stride, "workspace_bytes": ws.numel()}
    for name, call in (("jpeg_encode_two_launches", lambda: _jpeg.encode(src, rows, quality, sub, out, stride, lengths, ws)),
                       ("torch_copy_same_bytes", lambda: b.copy_(a)),
                       ("jpeg_encode_two_launches_again", lambda: _jpeg.encode(src, rows, quality, sub, out, stride, lengths, ws)),
                       ("torch_copy_same_bytes_again", lambda: b.copy_(a))):
        us = _event_us_each(call, launches=100, warmup=10)
        rec[name] = {"us_per_call_median": us, "gb_per_s": round(moved / us / 1e3, 1)}
    try:
        import io

        from PIL import Image
    except ImportError:
        rec["pillow_host_encode_ms"] = None
    else:
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            Image.fromarray(frames[0]).save(io.BytesIO(), "JPEG", quality=quality, subsampling=2 if subsampling == "420" else 0)
            times.append(time.perf_counter() - t0)
        rec["pillow_host_encode_ms"] = round(min(times) * 1e3, 2)
    return rec


def vis_files_record(inf, fmt, n_images, repeats, bs=8):
    """images/s of `Inferencer(visualizer={}, vis_format=fmt)(frames, out_dir=<tmpfs>)` on 1920x1080 frames at batch_size
    8, fp16, against the same call of an Inferencer without a visualiser, alternating; with fmt 'jpeg' also the encoder's
    own time.  Random weights draw few boxes: the encoder's work depends on the image, not on the box count."""
    import bench
    from codetr.inferencer import Inferencer

    frames = vis_frames(n_images)
    plain = Inferencer(inf.model, bench.CFG, dataset_meta=None)
    v = Inferencer(inf.model, bench.CFG, dataset_meta=None, visualizer={}, vis_format=fmt)
    root = tempfile.mkdtemp(prefix="bench_vis_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rec = {"vis_format": fmt, "batch_size": bs, "images": n_images, "frame_wh": [1920, 1080], "repeats": repeats,
           "dtype": "fp16", "out_dir": "tmpfs" if root.startswith("/dev/shm") else "temporary directory"}
    try:
        for name, who in (("no_visualisation", plain), ("out_dir_vis", v), ("no_visualisation_again", plain),
                          ("out_dir_vis_again", v)):
            kw = dict(out_dir=os.path.join(root, name)) if who is v else {}
            with torch.no_grad():
                who(frames[:bs], device=DEV, dtype=torch.float16, batch_size=bs, **kw)   # warm-up
                times = []
                for _ in range(repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = who(frames, device=DEV, dtype=torch.float16, batch_size=bs, **kw)
                    times.append(time.perf_counter() - t0)
            rec[name] = {"images_per_s": round(n_images / min(times), 2), "pass_s": [round(t, 4) for t in times]}
            if who is v:
                files = sorted(os.listdir(os.path.join(root, name, "vis")))
                rec[name]["files"] = len(files)
                rec[name]["file_bytes_mean"] = int(np.mean([os.path.getsize(os.path.join(root, name, "vis", f)) for f in files]))
                rec[name]["first_file"] = files[0]
        rec["detections_per_image"] = round(sum(len(p["labels"]) for p in out["predictions"]) / n_images, 1)
        rec["drawn_above_0.3_per_image"] = round(sum(sum(s > 0.3 for s in p["scores"]) for p in out["predictions"]) / n_images, 1)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if fmt == "jpeg":
        rec["encoder"] = jpeg_kernel_times(frames[:8], v.vis_format["quality"], v.vis_format["subsampling"])
    return rec


def redact_kernel_times(frames, Q=300, people=20, seed=11):
    """us per hip_ops.redact_detections call of every mode on the frames (one buffer) with `people` person-sized boxes of
    Q rows per frame above the threshold, beside a device-to-device copy of the buffer, draw_detections on the same
    operands, the same call with no selected row, and the numpy restatement of one frame on this machine's CPU"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import redact_ref

    from codetr import hip_ops
    from codetr.inferencer import generated_palette

    N, (H, W) = len(frames), frames[0].shape[:2]
    rng = np.random.default_rng(seed)
    boxes = np.zeros((N, Q, 4), np.float32)
    c = rng.uniform((0, 0), (W, H), (N, Q, 2))
    wh = np.stack((rng.uniform(60, 160, (N, Q)), rng.uniform(160, 420, (N, Q))), -1)      # persons: 60-160 x 160-420
    boxes[...] = np.concatenate((c - wh / 2, c + wh / 2), -1)
    scores = np.full((N, Q), 0.1, np.float32)
    scores[:, :people] = rng.uniform(0.4, 1.0, (N, people))
    labels = np.zeros((N, Q), np.int64)
    src = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(DEV)
    buf, other = src.clone(), torch.empty_like(src)
    rows = [(n * H * W * 3, H, W) for n in range(N)]
    dets = hip_ops.Detections(torch.from_numpy(boxes).half().to(DEV), torch.from_numpy(scores).half().to(DEV),
                              torch.from_numpy(labels).to(DEV), torch.full((N,), Q, dtype=torch.int32, device=DEV), None)
    none = torch.zeros(1, dtype=torch.uint8, device=DEV)   # label 0 is not selected: no row is
    names = hip_ops.draw_names_table(["person"]).to(DEV)
    colors = torch.tensor(generated_palette(1), dtype=torch.uint8, device=DEV)
    rec = {"frames": N, "frame_wh": [W, H], "Q": Q, "rows_above_threshold_per_frame": people, "buffer_bytes": src.numel(),
           "launches": 200, "timing": "HIP event pair around each call, median"}
    calls = [("torch_copy_buffer", lambda: other.copy_(buf)),
             ("draw_detections", lambda: hip_ops.draw_detections(buf, rows, dets, names, colors))]
    for mode in ("fill", "pixelate", "blur"):
        for shape in ("box", "ellipse"):
            st = dict(mode=mode, shape=shape)
            calls.append((f"redact_{mode}_{shape}", lambda st=st: hip_ops.redact_detections(buf, rows, dets, st)))
        calls.append((f"redact_{mode}_no_selected_row",
                      lambda st=dict(mode=mode): hip_ops.redact_detections(buf, rows, dets, st, none)))
    for again in ("", "_again"):
        for name, call in calls:
            buf.copy_(src)
            rec[name + again] = {"us_per_call_median": _event_us_each(call, launches=200, warmup=10)}
    buf.copy_(src)
    hip_ops.redact_detections(buf, rows, dets, dict(mode="blur"))
    got = buf[:H * W * 3].cpu().numpy().reshape(H, W, 3)
    t0 = time.perf_counter()
    ref, red = redact_ref.redact(frames[0], dets.boxes[0].float().cpu().numpy(), dets.scores[0].float().cpu().numpy(), labels[0],
                                 dict(mode="blur"))
    rec["numpy_restatement_blur_one_frame_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    rec["matches_restatement"] = bool(np.array_equal(got, ref))
    rec["masked_pixels_frame_0"] = int((ref != frames[0]).any(-1).sum())
    rec["redacted_rows_frame_0"] = len(red)
    return rec


def redact_record(inf, mode, n_images, repeats, bs=8):
    """the kernels alone (redact_kernel_times) and images/s of the Inferencer writing vis/%08d.jpg from 1920x1080 frames at
    batch_size 8, fp16, with and without redact=dict(mode=mode), alternating.  Random weights: the record says how many rows
    a frame had redacted."""
    import bench
    from codetr.inferencer import Inferencer

    frames = vis_frames(n_images)
    kw = dict(dataset_meta=None, visualizer={}, vis_format="jpeg")
    off, on = Inferencer(inf.model, bench.CFG, **kw), Inferencer(inf.model, bench.CFG, redact=dict(mode=mode), **kw)
    root = tempfile.mkdtemp(prefix="bench_redact_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rec = {"mode": mode, "batch_size": bs, "images": n_images, "frame_wh": [1920, 1080], "repeats": repeats, "dtype": "fp16",
           "vis_format": "jpeg", "out_dir": "tmpfs" if root.startswith("/dev/shm") else "temporary directory"}
    try:
        for name, who in (("vis_jpeg", off), ("vis_jpeg_redact", on), ("vis_jpeg_again", off), ("vis_jpeg_redact_again", on)):
            with torch.no_grad():
                who(frames[:bs], device=DEV, dtype=torch.float16, batch_size=bs, out_dir=os.path.join(root, name))   # warm-up
                times = []
                for _ in range(repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = who(frames, device=DEV, dtype=torch.float16, batch_size=bs, out_dir=os.path.join(root, name))
                    times.append(time.perf_counter() - t0)
            rec[name] = {"images_per_s": round(n_images / min(times), 2), "pass_s": [round(t, 4) for t in times]}
            if who is on:
                rec["redacted_rows_per_image"] = round(sum(len(p["redacted"]) for p in out["predictions"]) / n_images, 1)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    rec["kernels"] = redact_kernel_times(frames[:8])
    return rec


FRAME_WH = (1920, 1080)


def frame_items(fmt, n, seed=7):
    """n random 1920x1080 frames of the format as decoders hand them out, and their RGB conversion (tests/frames_ref.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frames_ref

    rng = np.random.default_rng(seed)
    W, H = FRAME_WH
    items = [frames_ref.item(fmt, H, W, frames_ref.random_planes(fmt, H, W, rng)) for _ in range(n)]
    return items, [frames_ref.to_rgb(it, fmt) for it in items]


def _event_us_each(call, launches=200, warmup=20):
    """median us of one launch, an event pair around each: what the GPU spends on it, whatever the host takes to enqueue"""
    for _ in range(warmup):
        call()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    torch.cuda.synchronize()
    for t0, t1 in pairs:
        t0.record()
        call()
        t1.record()
    torch.cuda.synchronize()
    return round(float(np.median([t0.elapsed_time(t1) for t0, t1 in pairs])) * 1e3, 2)


def frames_kernel_times(fmt, N=8):
    """us per launch of frames_to_rgb_kernel on N 1920x1080 frames (planes packed, 16-byte aligned, as stage_chunk lays
    them out) and of a device-to-device copy of as many bytes as the kernel reads and writes together"""
    from codetr import hip_ops

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frames_ref

    W, H = FRAME_WH
    rows, at, dst = [], 0, 0
    for _ in range(N):
        cols = []
        for r, rb in frames_ref.plane_shapes(fmt, H, W):
            at = -(-at // 16) * 16
            cols += [at, rb]
            at += r * rb
        rows.append((fmt, H, W) + tuple(cols) + (0,) * (6 - len(cols)) + (dst,))
        dst = -(-(dst + H * W * 3) // 16) * 16
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (at,), dtype=torch.uint8, generator=g).to(DEV)
    out = torch.empty((dst,), dtype=torch.uint8, device=DEV)
    moved = at + N * H * W * 3
    a, b = torch.randint(0, 256, (moved // 2,), dtype=torch.uint8, generator=g).to(DEV), torch.empty((moved // 2,),
                                                                                                   dtype=torch.uint8, device=DEV)
    rec = {"frames": N, "frame_wh": list(FRAME_WH), "format": fmt, "bytes_read": at, "bytes_written": N * H * W * 3}
    for name, call in (("frames_to_rgb_kernel", lambda: hip_ops.frames_to_rgb(src, rows, dst, out=out)),
                       ("torch_copy_same_bytes", lambda: b.copy_(a)),
                       ("frames_to_rgb_kernel_again", lambda: hip_ops.frames_to_rgb(src, rows, dst, out=out)),
                       ("torch_copy_same_bytes_again", lambda: b.copy_(a))):
        us = _event_us_each(call)
        rec[name] = {"us_per_launch_median": us, "gb_per_s": round(moved / us / 1e3, 1)}
    return rec


def frames_record(inf, fmt, n_images, repeats, resident, bs=8):
    items, rgb = frame_items(fmt, n_images)
    rec = {"format": fmt, "batch_size": bs, "images": n_images, "frame_wh": list(FRAME_WH), "repeats": repeats,
           "dtype": "fp16", "kernel": frames_kernel_times(fmt)}
    arms = {f"{fmt}_from_host": (items, fmt), "rgb_preconverted_from_host": (rgb, "rgb")}
    if resident:
        on_gpu = [torch.from_numpy(np.ascontiguousarray(it)).to(DEV) for it in items]   # (1920x1080: one array per frame)
        arms[f"{fmt}_gpu_resident"] = (on_gpu, fmt)
    for name in arms:
        rec[name] = {"pass_s": []}
    with torch.no_grad():
        for frames, f in arms.values():
            inf(frames[:bs], device=DEV, dtype=torch.float16, batch_size=bs, input_format=f)     # warm-up
        for _ in range(3):                                                                        # the arms in turn
            for name, (frames, f) in arms.items():
                for _ in range(repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    inf(frames, device=DEV, dtype=torch.float16, batch_size=bs, input_format=f)
                    rec[name]["pass_s"].append(round(time.perf_counter() - t0, 4))
    for name in arms:
        rec[name]["images_per_s"] = round(n_images / min(rec[name]["pass_s"]), 2)
        rec[name]["images_per_s_median"] = round(n_images / float(np.median(rec[name]["pass_s"])), 2)
    return rec


def decode_files(frames, quality=90):
    """the frames as JPEG files: written by Pillow where it imports (4:2:0, no restart markers: what a camera or a file
    on disk looks like), else by the project's own GPU encoder (one restart interval per MCU row) -> (files, writer)"""
    from codetr import hip_ops

    try:
        import io

        from PIL import Image
    except ImportError:
        flat = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(DEV)
        offs = np.cumsum([0] + [f.size for f in frames]).tolist()
        return hip_ops.encode_jpeg(flat, [(o, f.shape[0], f.shape[1]) for o, f in zip(offs, frames)], quality, "420"), "encode_jpeg"
    files = []
    for f in frames:
        b = io.BytesIO()
        Image.fromarray(f).save(b, "JPEG", quality=quality, subsampling=2)
        files.append(b.getvalue())
    return files, "pillow"


def decode_record(inf, n_images, repeats, bs=8):
    """`--decode jpeg`: the Inferencer fed JPEG files (decoded on the GPU) against the same frames decoded on the host by
    Pillow in front of the call and against frames that are already arrays; the decoder's launches alone; the bytes of
    the upload either way"""
    from codetr import hip_ops

    frames = vis_frames(n_images)
    files, writer = decode_files(frames)
    rec = {"batch_size": bs, "images": n_images, "frame_wh": list(FRAME_WH), "repeats": repeats, "dtype": "fp16",
           "files_written_by": writer, "file_bytes_mean": int(np.mean([len(f) for f in files])),
           "raw_bytes": int(frames[0].size), "info": hip_ops.jpeg_info(files[0])}
    # the launches alone: eight files, staged once
    parsed = []
    for f in files[:8]:
        data = hip_ops.jpeg_file_bytes(f)
        rc, info, tables = hip_ops.jpeg_parse(data)
        assert rc == 0, hip_ops.jpeg_reason(rc, info)
        parsed.append((data, info, tables))
    copies, groups, scan_at, end = hip_ops.jpeg_stage(parsed)
    host = np.zeros(end, np.uint8)
    for at, part in copies:
        host[at:at + part.size] = part
    up = torch.from_numpy(host).to(DEV)
    offs = [k * (-(-frames[0].size // 16) * 16) for k in range(len(parsed))]
    dst = torch.empty((offs[-1] + frames[0].size,), dtype=torch.uint8, device=DEV)
    us = _event_us_each(lambda: hip_ops.jpeg_decode_staged(up, parsed, groups, scan_at, offs, dst), launches=50, warmup=5)
    rec["kernels"] = {"files": len(parsed), "us_per_call_median": us, "us_per_frame": round(us / len(parsed), 1),
                      "bytes_uploaded": int(end), "bytes_written": int(len(parsed) * frames[0].size)}
    t0 = time.perf_counter()
    for f in files[:8]:
        hip_ops.jpeg_parse(hip_ops.jpeg_file_bytes(f))
    rec["host_parse_us_per_file"] = round((time.perf_counter() - t0) / 8 * 1e6, 1)
    arms = {"jpeg_decoded_on_gpu": lambda: inf(files, device=DEV, dtype=torch.float16, batch_size=bs, input_format="jpeg"),
            "arrays_already_decoded": lambda: inf(frames, device=DEV, dtype=torch.float16, batch_size=bs)}
    if writer == "pillow":
        import io

        from PIL import Image

        def host_decoded():
            return inf([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files], device=DEV, dtype=torch.float16,
                       batch_size=bs)

        arms["jpeg_decoded_by_pillow_on_host"] = host_decoded
        t0 = time.perf_counter()
        for f in files[:8]:
            np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        rec["pillow_decode_ms_per_frame"] = round((time.perf_counter() - t0) / 8 * 1e3, 2)
    for name in arms:
        rec[name] = {"pass_s": []}
    with torch.no_grad():
        for call in arms.values():
            call()                                             # warm-up
        for _ in range(3):                                     # the arms in turn
            for name, call in arms.items():
                for _ in range(repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    rec[name]["pass_s"].append(round(time.perf_counter() - t0, 4))
    for name in arms:
        rec[name]["images_per_s"] = round(n_images / min(rec[name]["pass_s"]), 2)
        rec[name]["images_per_s_median"] = round(n_images / float(np.median(rec[name]["pass_s"])), 2)
    return rec


def track_detections(frames, Q=300, objects=100, seed=5):
    """`frames` frames of Q fp16 detection rows: `objects` boxes on slow straight paths with jitter (score 0.75..0.95, five
    labels), the other rows clutter of score 0.15..0.55 -> hip_ops.Detections on the device"""
    from codetr import hip_ops

    rng = np.random.default_rng(seed)
    c0, wh = rng.uniform(60, 1800, (objects, 2)), rng.uniform(40, 120, (objects, 2))
    v = rng.uniform(-1.5, 1.5, (objects, 2))
    boxes, scores = np.zeros((frames, Q, 4), np.float32), np.zeros((frames, Q), np.float32)
    for f in range(frames):
        c = c0 + v * f + rng.uniform(-1, 1, (objects, 2))
        boxes[f, :objects] = np.concatenate((c - wh / 2, c + wh / 2), 1)
        scores[f, :objects] = rng.uniform(0.75, 0.95, objects)
        cc, cw = rng.uniform(0, 1900, (Q - objects, 2)), rng.uniform(10, 80, (Q - objects, 2))
        boxes[f, objects:] = np.concatenate((cc, cc + cw), 1)
        scores[f, objects:] = rng.uniform(0.15, 0.55, Q - objects)
    labels = np.tile(np.arange(Q) % 5, (frames, 1))
    return hip_ops.Detections(torch.tensor(boxes).half().to(DEV), torch.tensor(scores).half().to(DEV),
                              torch.tensor(labels).to(DEV), torch.full((frames,), Q, dtype=torch.int32, device=DEV), None)


def crowd_detections(frames, Q=300, objects=100, seed=9, side=350.0):
    """`frames` frames of Q fp16 rows: `objects` boxes of about 90 x 150 of ONE label wandering inside a side x side
    square, so that every box overlaps many others (the workload on which the associations differ), the other rows
    low-score clutter in the same square -> (hip_ops.Detections on the device, the same arrays on the host)"""
    from codetr import hip_ops

    rng = np.random.default_rng(seed)
    c0, wh = rng.uniform(0, side, (objects, 2)), rng.uniform((80, 130), (100, 170), (objects, 2))
    v = rng.uniform(-8, 8, (objects, 2))
    boxes, scores = np.zeros((frames, Q, 4), np.float32), np.zeros((frames, Q), np.float32)
    for f in range(frames):
        c = c0 + v * f + rng.uniform(-4, 4, (objects, 2))
        boxes[f, :objects] = np.concatenate((c - wh / 2, c + wh / 2), 1)
        scores[f, :objects] = rng.uniform(0.75, 0.95, objects)
        cc, cw = rng.uniform(0, side, (Q - objects, 2)), rng.uniform(40, 120, (Q - objects, 2))
        boxes[f, objects:] = np.concatenate((cc, cc + cw), 1)
        scores[f, objects:] = rng.uniform(0.15, 0.55, Q - objects)
    labels = np.zeros((frames, Q), np.int64)
    b16, s16 = torch.tensor(boxes).half(), torch.tensor(scores).half()
    dets = hip_ops.Detections(b16.to(DEV), s16.to(DEV), torch.tensor(labels).to(DEV),
                              torch.full((frames,), Q, dtype=torch.int32, device=DEV), None)
    return dets, (b16, s16, labels)


def track_kernel_times(Q=300, objects=100):
    """us per launch of the tracking kernels, greedy (track_kernel<false, ..>) and optimal (track_kernel<true, 0, ..>) alternating
    in one session: 8 frames of one stream, one frame of each of 8 streams, and 8 frames of a crowd of overlapping
    objects; the states hold about `objects` live tracks (8 frames are walked before the clock starts).  For the crowd
    the restatements (tests/) give the solver's rounds per frame and the frames on which the two associations differ."""
    from codetr import hip_ops

    dets = track_detections(8, Q, objects)
    crowd, crowd_host = crowd_detections(16, Q, objects)
    first, second = [hip_ops.Detections(*(None if t is None else t[i:i + 8] for t in crowd)) for i in (0, 8)]
    rec = {"Q": Q, "objects": objects}
    # crowd_replayed: the chunk shown a second time, i.e. every object jumps back by 8 frames of its motion at once -- a
    # cut in the video; the tracks no longer sit on their objects and the augmenting paths grow long
    for name, streams, warm, timed in (("8_frames_of_1_stream", [0] * 8, [dets], dets),
                                       ("1_frame_of_8_streams", list(range(8)), [dets] * 8, dets),
                                       ("crowd_8_frames_of_1_stream", [0] * 8, [first], second),
                                       ("crowd_replayed_8_frames_of_1_stream", [0] * 8, [first, second], second)):
        rec[name] = {}
        states, keeps = {}, {}
        for association in hip_ops.TRACK_ASSOCIATIONS:
            states[association] = state = hip_ops.new_track_state(8, hip_ops.TRACKER["max_tracks"], DEV)
            for chunk in warm:
                hip_ops.track_update(chunk, state, streams, association=association)
            keeps[association] = state.clone()
        for turn in range(2):                                                 # greedy and optimal alternating
            for association in hip_ops.TRACK_ASSOCIATIONS:
                state, keep = states[association], keeps[association]

                def timed_call():
                    hip_ops.track_update(timed, state, streams, association=association)

                if timed is dets:         # r17's workloads: the state moves on from launch to launch, as r17 measured
                    us = _event_us_each(timed_call, launches=100, warmup=5)
                else:
                    us = _track_us_restoring(state, keep, timed_call)
                host = hip_ops.track_state_to_host(state)
                rec[name].setdefault(association, {"us_per_launch_median": []})["us_per_launch_median"].append(us)
                rec[name][association]["live_tracks_per_stream"] = int((host.id[0] != 0).sum())
    # the crowd through the two restatements: rounds per frame, and where the associations part ways
    import track_assign_ref
    import track_ref
    g, o = track_ref.TrackRef(), track_assign_ref.TrackAssignRef()
    rounds, differ, before = [], 0, 0
    for f in range(16):
        ids_g = g.update(crowd_host[0][f], crowd_host[1][f], crowd_host[2][f])
        ids_o = o.update(crowd_host[0][f], crowd_host[1][f], crowd_host[2][f])
        differ += int(f >= 8 and not np.array_equal(ids_g, ids_o))
        rounds.append(o.log["rounds"] - before)
        before = o.log["rounds"]
    rec["crowd_8_frames_of_1_stream"]["solver_rounds_per_frame"] = rounds[8:]
    rec["crowd_8_frames_of_1_stream"]["frames_where_greedy_and_optimal_differ"] = differ
    rounds = []
    for f in range(8, 16):
        o.update(crowd_host[0][f], crowd_host[1][f], crowd_host[2][f])
        rounds.append(o.log["rounds"] - before)
        before = o.log["rounds"]
    rec["crowd_replayed_8_frames_of_1_stream"]["solver_rounds_per_frame"] = rounds
    o2 = track_assign_ref.TrackAssignRef()
    h = [t.cpu() if torch.is_tensor(t) else t for t in (dets.boxes, dets.scores, dets.labels)]
    for _ in range(2):
        before = o2.log["rounds"]
        for f in range(8):
            o2.update(h[0][f], h[1][f], h[2][f].numpy())
    rec["8_frames_of_1_stream"]["solver_rounds_per_launch"] = o2.log["rounds"] - before
    return rec


def _track_us_restoring(state, keep, call, launches=50, warmup=3):
    """median us of one launch that always starts from the state `keep` (restored outside the event pair)"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for i in range(warmup + launches):
        state.copy_(keep)
        if i >= warmup:
            pairs[i - warmup][0].record()
        call()
        if i >= warmup:
            pairs[i - warmup][1].record()
    torch.cuda.synchronize()
    return round(float(np.median([t0.elapsed_time(t1) for t0, t1 in pairs])) * 1e3, 2)


def assign_times():
    """codetr_assign_i32 beside scipy.optimize.linear_sum_assignment on this box's CPU: 100 x 900 (a DETR matcher's
    shape; gains at 10 % density) with B = 8, and 300 x 300 dense; us per launch (event pairs, median) / per call"""
    from scipy.optimize import linear_sum_assignment
    from codetr import hip_ops
    import assign_ref

    rng = np.random.default_rng(1)
    rec = {}
    for name, (B, n, m, density) in (("100x900_B8", (8, 100, 900, 0.1)), ("100x900_B8_dense", (8, 100, 900, 1.0)),
                                     ("300x300_dense", (1, 300, 300, 1.0))):
        G = rng.integers(1, hip_ops.ASSIGN_MAX_GAIN + 1, (B, n, m)) * (rng.random((B, n, m)) < density)
        dev = torch.tensor(G.astype(np.int32)).to(DEV)
        match, total = hip_ops.linear_assignment(dev)
        us = _event_us_each(lambda: hip_ops.linear_assignment(dev), launches=50, warmup=3)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            want = [int(G[b][linear_sum_assignment(G[b], maximize=True)].sum()) for b in range(B)]
            t.append(time.perf_counter() - t0)
        rounds = [assign_ref.solve(G[b])[2] for b in range(B)]
        rec[name] = {"gpu_us_per_launch_median": us, "scipy_us_median": round(float(np.median(t)) * 1e6, 1),
                     "totals_equal_scipy": total.tolist() == want, "rounds_per_problem": rounds,
                     "gpu_us_per_round_of_the_longest": round(us / max(rounds), 3)}
    return rec


def track_record(inf, images, repeats, bs=8):
    """images/s of the Inferencer on `images` as one stream: with the tracker, without it, and with the host composition
    the tracker replaces -- the untracked call's predictions through tests/track_ref.py frame by frame, state on the host"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_ref
    from codetr.inferencer import Inferencer

    tracked = Inferencer(inf.model, bench_cfg(), dataset_meta=None, tracker={})
    optimal = Inferencer(inf.model, bench_cfg(), dataset_meta=None, tracker={}, track_association="optimal")
    rec = {"batch_size": bs, "images": len(images), "repeats": repeats, "dtype": "fp16", "kernel": track_kernel_times(),
           "assign": assign_times()}
    host_ref = [None]

    def with_tracker():
        tracked.reset_tracks()
        return tracked(images, device=DEV, dtype=torch.float16, batch_size=bs)["predictions"]

    def with_tracker_optimal():
        optimal.reset_tracks()
        return optimal(images, device=DEV, dtype=torch.float16, batch_size=bs)["predictions"]

    def without():
        return inf(images, device=DEV, dtype=torch.float16, batch_size=bs)["predictions"]

    def host_composition():
        host_ref[0] = ref = track_ref.TrackRef()
        preds = without()
        for p in preds:
            n = len(p["labels"])
            p["track_ids"] = ref.update(np.asarray(p["bboxes"], np.float32).reshape(n, 4), np.asarray(p["scores"], np.float32),
                                        np.asarray(p["labels"], np.int64)).tolist()
        return preds

    arms = {"with_tracker": with_tracker, "with_tracker_optimal": with_tracker_optimal, "without_tracker": without,
            "host_composition": host_composition}
    for name in arms:
        rec[name] = {"pass_s": []}
    with torch.no_grad():
        got = {name: call() for name, call in arms.items()}                                   # warm-up
        rec["ids_equal_host_composition"] = [p["track_ids"] for p in got["with_tracker"]] == \
            [p["track_ids"] for p in got["host_composition"]]
        rec["detections_per_image"] = round(float(np.mean([len(p["labels"]) for p in got["without_tracker"]])), 1)
        rec["tracks_started"] = int(host_ref[0].state().next_id - 1)
        for _ in range(3):                                                                    # the arms in turn
            for name, call in arms.items():
                for _ in range(repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    rec[name]["pass_s"].append(round(time.perf_counter() - t0, 4))
    for name in arms:
        rec[name]["images_per_s"] = round(len(images) / min(rec[name]["pass_s"]), 2)
        rec[name]["images_per_s_median"] = round(len(images) / float(np.median(rec[name]["pass_s"])), 2)
    return rec


def motion_record(inf, repeats, bs=8, frames=16, model="translation"):
    """camera-motion compensation (`--track --motion`): estimate_motion alone on 8 frames of 1920 x 1080 beside a
    device-to-device copy of the same bytes (HIP events, 200 launches); track_update on the --track workloads with and
    without a motion operand, alternating; the tracked Inferencer on panned 1920 x 1080 frames as one stream with and
    without track_motion, the two in turn, three times.  model="similarity" (`--motion similarity`): the estimate's
    five-launch form beside the three-launch one (the difference is the two launches of the fit), the five-launch form on
    8 frames of 320 x 320 with all 81 blocks textured (the largest search there is), track_update with [N, 8] against
    [N, 4] rows, and a third Inferencer arm"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import motion_cases
    from codetr import hip_ops
    from codetr.inferencer import Inferencer

    H, W, margin = 1080, 1920, 128
    canvas = motion_cases.texture(5, H + 2 * margin, W + 2 * margin, 48)
    rng = np.random.default_rng(9)
    pans = [(0, 0)] + [(int(rng.integers(-60, 61)), int(rng.integers(-40, 41))) for _ in range(frames - 1)]
    shifts, x, y = [], 0, 0
    for dx, dy in pans:   # (a walk that stays inside the canvas margin)
        dx = -dx if abs(x + dx) > margin else dx
        dy = -dy if abs(y + dy) > margin else dy
        x, y = x + dx, y + dy
        shifts.append((x, y))
    images = [motion_cases.view(canvas, (H, W), s, margin) for s in shifts]
    rec = {"frames": frames, "frame_hw": [H, W], "batch_size": bs, "dtype": "fp16"}

    buf = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images[:8]])).to(DEV)
    rows = [(i * H * W * 3, H, W) for i in range(8)]
    state = hip_ops.new_motion_state(1, DEV)
    motion, diag = hip_ops.estimate_motion(buf, rows, state)
    dst = torch.empty_like(buf)
    rec["estimate"] = {"bytes": buf.numel(), "motion": motion.cpu().tolist(), "diag": diag.cpu().tolist(),
                       "true_pans": [[shifts[i][0] - shifts[i - 1][0], shifts[i][1] - shifts[i - 1][1]] for i in range(1, 8)],
                       "us_per_call_median": [], "copy_us_median": []}
    sim = model == "similarity"
    if sim:
        motion8, diag8 = hip_ops.estimate_motion(buf, rows, state, model="similarity")
        rec["estimate"].update({"similarity_motion": motion8.cpu().tolist(), "similarity_diag": diag8.cpu().tolist(),
                                "similarity_us_per_call_median": [], "similarity_81_blocks_us_median": [],
                                "translation_81_blocks_us_median": []})
        fine = motion_cases.texture(5, 320 + 2 * margin, 320 + 2 * margin, 12)   # (fine enough that every block is textured)
        small = [motion_cases.view(fine, (320, 320), (s[0] // 8, s[1] // 8), margin) for s in shifts[:8]]
        buf81 = torch.from_numpy(np.concatenate([im.reshape(-1) for im in small])).to(DEV)
        rows81 = [(i * 320 * 320 * 3, 320, 320) for i in range(8)]
        state81 = hip_ops.new_motion_state(1, DEV)
        rec["estimate"]["diag_81_blocks"] = hip_ops.estimate_motion(buf81, rows81, state81, model="similarity")[1].cpu().tolist()
    for _ in range(3):                                                        # in turn
        rec["estimate"]["us_per_call_median"].append(_event_us_each(lambda: hip_ops.estimate_motion(buf, rows, state)))
        if sim:
            rec["estimate"]["similarity_us_per_call_median"].append(
                _event_us_each(lambda: hip_ops.estimate_motion(buf, rows, state, model="similarity")))
            rec["estimate"]["similarity_81_blocks_us_median"].append(
                _event_us_each(lambda: hip_ops.estimate_motion(buf81, rows81, state81, model="similarity")))
            rec["estimate"]["translation_81_blocks_us_median"].append(
                _event_us_each(lambda: hip_ops.estimate_motion(buf81, rows81, state81)))
        rec["estimate"]["copy_us_median"].append(_event_us_each(lambda: dst.copy_(buf)))

    dets = track_detections(8, 300, 100)
    moved = torch.tensor([[3.5, -2.25, 1.0, 0.0]] * 8, dtype=torch.float32, device=DEV)
    turned = torch.tensor([[3.5, -2.25, 1.0, 2.0, 1.0, 0.0, 960.0, 540.0]] * 8, dtype=torch.float32, device=DEV)
    operands = [("without_motion_us", None), ("with_motion_us", moved)] + ([("with_similarity_us", turned)] if sim else [])
    rec["track_update"] = {}
    for name, streams in (("8_frames_of_1_stream", [0] * 8), ("1_frame_of_8_streams", list(range(8)))):
        rec["track_update"][name] = {key: [] for key, _ in operands}
        states = {}
        for key, _ in operands:
            states[key] = hip_ops.new_track_state(8, hip_ops.TRACKER["max_tracks"], DEV)
            for _ in range(1 if name[0] == "8" else 8):
                hip_ops.track_update(dets, states[key], streams)
        for _ in range(3):
            for key, m in operands:
                rec["track_update"][name][key].append(
                    _event_us_each(lambda: hip_ops.track_update(dets, states[key], streams, motion=m), launches=100, warmup=5))

    arms = {"tracker": Inferencer(inf.model, bench_cfg(), dataset_meta=None, tracker={}),
            "tracker_and_motion": Inferencer(inf.model, bench_cfg(), dataset_meta=None, tracker={}, track_motion="translation")}
    if sim:
        arms["tracker_and_similarity"] = Inferencer(inf.model, bench_cfg(), dataset_meta=None, tracker={},
                                                    track_motion="similarity")
    for name in arms:
        rec[name] = {"pass_s": []}
    with torch.no_grad():
        for name, arm in arms.items():                                        # warm-up
            got = arm(images, device=DEV, dtype=torch.float16, batch_size=bs)["predictions"]
            if name == "tracker_and_motion":
                rec["camera_motion_first_8"] = [p["camera_motion"] for p in got[:8]]
        for _ in range(3):
            for name, arm in arms.items():
                for _ in range(repeats):
                    arm.reset_tracks()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    arm(images, device=DEV, dtype=torch.float16, batch_size=bs)
                    rec[name]["pass_s"].append(round(time.perf_counter() - t0, 4))
    for name in arms:
        rec[name]["images_per_s"] = round(len(images) / min(rec[name]["pass_s"]), 2)
        rec[name]["images_per_s_median"] = round(len(images) / float(np.median(rec[name]["pass_s"])), 2)
    return rec


def appearance_record(inf, repeats, bs=8, frames=16):
    """the appearance cue (`--track --appearance`): appearance_descriptors alone at N = 8, Q = 300 on 1920 x 1080 frames
    beside a device-to-device copy of the bytes it reads (the sampled pixels: 512 x 3 bytes per participating row; HIP
    events, 200 launches); track_update on the --track workload (300 rows, 100 live tracks) with and without the operand,
    greedy and optimal, alternating; the tracked Inferencer at batch_size 8 over 16 frames of 1920 x 1080 as one stream
    with and without track_appearance, the two in turn, three times"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import motion_cases
    from codetr import hip_ops
    from codetr.inferencer import Inferencer

    H, W, margin = 1080, 1920, 16
    canvas = motion_cases.texture(5, H + 2 * margin, W + 2 * margin, 48)
    images = [motion_cases.view(canvas, (H, W), (f % 8, f % 5), margin) for f in range(frames)]
    rec = {"frames": frames, "frame_hw": [H, W], "batch_size": bs, "dtype": "fp16"}

    buf = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images[:8]])).to(DEV)
    rows = [(i * H * W * 3, H, W) for i in range(8)]
    dets = track_detections(8, 300, 100)
    desc = hip_ops.appearance_descriptors(buf, rows, dets)
    participating = int((desc.view(8, 300, -1).sum(dim=2) != 0).sum())
    read = torch.empty(participating * 512 * 3, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(read)
    rec["describe"] = {"rows": [8, 300], "participating_rows": participating, "bytes_read": read.numel(),
                       "bytes_written": desc.numel() * 2, "us_per_call_median": [], "copy_us_median": []}
    for _ in range(3):                                                        # in turn
        rec["describe"]["us_per_call_median"].append(_event_us_each(lambda: hip_ops.appearance_descriptors(buf, rows, dets)))
        rec["describe"]["copy_us_median"].append(_event_us_each(lambda: dst.copy_(read)))

    T = hip_ops.TRACKER["max_tracks"]
    rec["track_update"] = {}
    for name, streams in (("8_frames_of_1_stream", [0] * 8), ("1_frame_of_8_streams", list(range(8)))):
        rec["track_update"][name] = {}
        for association in hip_ops.TRACK_ASSOCIATIONS:
            arm = rec["track_update"][name][association] = {"without_appearance_us": [], "with_appearance_us": []}
            states = {key: hip_ops.new_track_state(8, T, DEV) for key in arm}
            astate = hip_ops.new_appearance_state(8, T, DEV)
            kws = {"without_appearance_us": {}, "with_appearance_us": dict(appearance=desc, appearance_state=astate)}
            for key in arm:
                for _ in range(1 if name[0] == "8" else 8):
                    hip_ops.track_update(dets, states[key], streams, association=association, **kws[key])
            for _ in range(3):
                for key in arm:
                    arm[key].append(_event_us_each(
                        lambda: hip_ops.track_update(dets, states[key], streams, association=association, **kws[key]),
                        launches=100, warmup=5))
            host = hip_ops.track_state_to_host(states["with_appearance_us"])
            arm["live_tracks_per_stream"] = int((host.id[0] != 0).sum())

    arms = {"tracker": Inferencer(inf.model, bench_cfg(), dataset_meta=None, tracker={}),
            "tracker_and_appearance": Inferencer(inf.model, bench_cfg(), dataset_meta=None, tracker={},
                                                 track_appearance="color")}
    for name in arms:
        rec[name] = {"pass_s": []}
    with torch.no_grad():
        for name, arm in arms.items():                                        # warm-up
            got = arm(images, device=DEV, dtype=torch.float16, batch_size=bs)["predictions"]
            rec[name]["detections_per_image"] = round(float(np.mean([len(p["labels"]) for p in got])), 1)
        for _ in range(3):
            for name, arm in arms.items():
                for _ in range(repeats):
                    arm.reset_tracks()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    arm(images, device=DEV, dtype=torch.float16, batch_size=bs)
                    rec[name]["pass_s"].append(round(time.perf_counter() - t0, 4))
    for name in arms:
        rec[name]["images_per_s"] = round(len(images) / min(rec[name]["pass_s"]), 2)
        rec[name]["images_per_s_median"] = round(len(images) / float(np.median(rec[name]["pass_s"])), 2)
    return rec


def bench_cfg():
    import bench

    return bench.CFG


def soft_inferencer(inf):
    """the same model behind the post-processing its config specifies (soft-NMS, max_per_img)"""
    import bench
    from codetr.inferencer import Inferencer

    return Inferencer(inf.model, bench.CFG, dataset_meta=None, nms_type="config")


def child(n_batch=16, n_single=4):
    """the workload traced by rocprofv3"""
    images = synthetic_images(n_batch, seed=1)
    for name, inf in inferencers().items():
        inf(images[:8], device=DEV, dtype=DTYPES[name], batch_size=8)   # warm-up
        inf(images, device=DEV, dtype=DTYPES[name], batch_size=8)
        if name == "fp16":
            inf(images[:n_single], device=DEV, dtype=torch.float16, batch_size=1)
            soft = soft_inferencer(inf)
            soft(images, device=DEV, dtype=torch.float16, batch_size=8)
    torch.cuda.synchronize()


def _kernel_key(name):
    """'postprocess_kernel<bf16>' etc. for the kernels of csrc/prepost.hip (demangled or mangled names), else None"""
    base = next((k for k in KERNELS if k in name), None)   # (KERNELS lists preprocess_batch_kernel first)
    if base is None or base == "batched_nms_kernel":
        return base
    dt = "bf16" if "Bf16" in name else "f16" if ("_Float16" in name or "DF16_" in name) else "f32"
    return f"{base}<{dt}>"


def profile(timeout_s=900):
    """run `child()` under rocprofv3 and fold its kernel statistics for the four pre / post kernels"""
    rocprof = shutil.which("rocprofv3")
    if rocprof is None:
        return {"error": "rocprofv3 not found"}
    out_dir = tempfile.mkdtemp(prefix="bench_inferencer_prof_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--",
               sys.executable, os.path.abspath(__file__), "--child"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout_s)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not stats:
            return {"error": f"rocprofv3 run failed (exit {r.returncode})", "tail": r.stdout[-2000:]}
        folded = {}
        for row in csv.DictReader(open(stats[0])):
            key = _kernel_key(row["Name"])
            if key is None:
                continue
            f = folded.setdefault(key, {"calls": 0, "total_us": 0.0})
            f["calls"] += int(row["Calls"])
            f["total_us"] += float(row["TotalDurationNs"]) / 1e3
        for f in folded.values():
            f["avg_us"] = round(f["total_us"] / max(1, f["calls"]), 2)
            f["total_us"] = round(f["total_us"], 2)
        return {"command": "rocprofv3 --kernel-trace --stats -- python tools/bench_inferencer.py --child",
                "workload": "per dtype: batch_size 8 over 16 images (+ one 8-image warm-up call); fp16 also batch_size 1 "
                            "over 4 images and nms_type='config' (soft-NMS) batch_size 8 over 16 images", "kernels": folded}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-sizes", default="1,4,8")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--tta", action="store_true", help="add the test-time-augmentation sub-record")
    ap.add_argument("--tta-images", type=int, default=8)
    ap.add_argument("--tta-only", action="store_true", help="only the tta sub-record (implies --tta)")
    ap.add_argument("--vis", nargs="?", const="on", choices=("on", "png", "jpeg"),
                    help="alone: add the visualisation sub-record; png | jpeg: only the record of the drawn files written "
                         "to an out_dir in that format (1920x1080 frames, batch_size 8, fp16)")
    ap.add_argument("--vis-only", action="store_true", help="only the vis sub-record (implies --vis)")
    ap.add_argument("--slice", action="store_true", help="add the sliced-inference sub-record")
    ap.add_argument("--slice-images", type=int, default=4)
    ap.add_argument("--slice-only", action="store_true", help="only the slice sub-record (implies --slice)")
    ap.add_argument("--frames", choices=("nv12", "i420", "bgr"), help="only the frames record, for frames of this format")
    ap.add_argument("--resident", action="store_true", help="with --frames: also feed the frames as GPU-resident tensors")
    ap.add_argument("--track", action="store_true", help="only the tracking record: the images as one stream")
    ap.add_argument("--motion", nargs="?", const="translation", choices=("translation", "similarity"),
                    help="with --track: only the camera-motion record (track_motion); similarity: with the similarity "
                         "model's arms beside the translation's")
    ap.add_argument("--appearance", action="store_true",
                    help="with --track: only the appearance record (track_appearance): the descriptors, the tracking "
                         "launch with and without them, the tracked Inferencer with and without the cue")
    ap.add_argument("--decode", choices=("jpeg",), help="only the record of JPEG files as input, decoded on the GPU")
    ap.add_argument("--redact", choices=("pixelate", "blur", "fill"),
                    help="only the redaction record: redact_detections alone per mode, and the Inferencer writing JPEG "
                         "files with and without redact=dict(mode=MODE)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inferencer: needs a GPU")
    if a.child:
        child()
        return
    images = synthetic_images(a.images)
    bss = [int(v) for v in a.batch_sizes.split(",")]
    res = {}
    infs = inferencers()
    if a.frames:
        print(json.dumps({"metric": "Inferencer on decoder frames (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock; HIP events for the kernel",
                          "frames": frames_record(infs["fp16"], a.frames, a.images, a.repeats, a.resident)}))
        return
    if a.decode:
        print(json.dumps({"metric": "Inferencer on JPEG files (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock; HIP events for the decoder",
                          "decode": decode_record(infs["fp16"], a.images, a.repeats)}))
        return
    if a.redact:
        print(json.dumps({"metric": "Inferencer redaction of detected regions (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock, best pass; HIP events for the kernels",
                          "redact": redact_record(infs["fp16"], a.redact, a.images, a.repeats)}))
        return
    if a.track and a.appearance:
        print(json.dumps({"metric": "Inferencer tracking with the appearance cue (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock; HIP events for the kernels",
                          "track_appearance": appearance_record(infs["fp16"], a.repeats)}))
        return
    if a.track and a.motion:
        print(json.dumps({"metric": "Inferencer tracking with camera-motion compensation (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock; HIP events for the kernels",
                          "track_motion": motion_record(infs["fp16"], a.repeats, model=a.motion)}))
        return
    if a.track:
        print(json.dumps({"metric": "Inferencer tracking (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock; HIP events for the kernel",
                          "track": track_record(infs["fp16"], images, a.repeats)}))
        return
    if a.tta_only:
        print(json.dumps({"metric": "Inferencer test-time augmentation (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock, best pass",
                          "tta": tta_record(infs["fp16"], a.tta_images, a.repeats)}))
        return
    if a.vis in ("png", "jpeg"):
        print(json.dumps({"metric": "Inferencer visualisation files (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock, best pass; HIP events for the encoder",
                          "vis_files": vis_files_record(infs["fp16"], a.vis, a.images, a.repeats)}))
        return
    if a.vis_only:
        print(json.dumps({"metric": "Inferencer visualisation (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock, best pass",
                          "vis": vis_record(infs["fp16"], images, a.repeats)}))
        return
    if a.slice_only:
        print(json.dumps({"metric": "Inferencer sliced inference (Swin-L config, random weights)",
                          "device": torch.cuda.get_device_name(0), "timing": "host clock, best pass",
                          "slice": slice_record(infs["fp16"], a.slice_images, a.repeats)}))
        return
    infs["fp16_soft_nms"] = soft_inferencer(infs["fp16"])
    for name, inf in infs.items():
        dt = DTYPES[name.split("_")[0]]
        res[name] = {}
        for bs in bss:
            with torch.no_grad():
                inf(images[:max(8, bs)], device=DEV, dtype=dt, batch_size=bs)   # warm-up: kernels, allocator, shapes
                best = None
                for _ in range(a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = inf(images, device=DEV, dtype=dt, batch_size=bs)
                    dt_s = time.perf_counter() - t0   # (ends with the detections on the host: no sync needed)
                    best = dt_s if best is None else min(best, dt_s)
            assert len(out["predictions"]) == len(images)
            res[name][f"batch_size_{bs}"] = round(len(images) / best, 2)
            print(f"[bench_inferencer] {name} batch_size {bs}: {res[name][f'batch_size_{bs}']} images/s", file=sys.stderr,
                  flush=True)
        if 1 in bss and 8 in bss:
            res[name]["speedup_8_vs_1"] = round(res[name]["batch_size_8"] / res[name]["batch_size_1"], 3)
    line = {"metric": "Inferencer images/s (Swin-L config, 1152x768 pipeline, random weights)", "unit": "images/s",
            "images": a.images, "image_sizes_wh": SIZES_WH, "repeats": a.repeats, "timing": "host clock, best pass",
            "device": torch.cuda.get_device_name(0), "results": res}
    line["postprocess_launch_us"] = post_kernel_times()
    if a.tta:
        line["tta"] = tta_record(infs["fp16"], a.tta_images, a.repeats)
    if a.vis:
        line["vis"] = vis_record(infs["fp16"], images, a.repeats)
    if a.slice:
        line["slice"] = slice_record(infs["fp16"], a.slice_images, a.repeats)
    if not a.no_profile:
        line["kernel_times"] = profile()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
