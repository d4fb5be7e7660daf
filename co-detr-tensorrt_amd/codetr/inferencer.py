"""``Inferencer`` -- the reference's image-in / detections-out wrapper (reference codetr/inferencer.py:27-499), with
its pre- and post-processing on the GPU.

Same constructor and call signature:
``Inferencer(model, model_file, dataset_meta, score_threshold=None, iou_threshold=None)`` reads ``score_thr`` /
``nms.iou_threshold`` from ``cfg.model.test_cfg[0]`` (reference :60-70), the mean / std of
``cfg.model.data_preprocessor`` (:72-76) and the ``Resize`` / ``Pad`` steps of the test pipeline (:95-101);
``__call__(images, ..., device, dtype)`` takes RGB ``np.ndarray`` images and returns
``{"predictions": [{"labels", "scores", "bboxes"}, ...], "visualization": []}`` (reference :402-485, ``pred2dict``
:303-341).  ``no_save_pred=False`` with an ``out_dir`` writes ``out_dir/preds/{num_predicted_imgs}.json`` per image, as
``pred2dict`` does.  Without a ``visualizer`` (below) ``return_vis`` raises; ``show`` and ``return_datasamples`` (a
window, mmengine's ``DetDataSample``) always do.

Per image (reference :441-452, :343-378): upload the uint8 image, one kernel for resize + pad + normalise + mask
(``hip_ops.preprocess_image``), ``model(batch_inputs, img_masks)``, score threshold, per-class NMS
(``hip_ops.batched_nms``), boxes / scale_factor.

``__call__(..., batch_size=B)`` with B > 1 (and any bf16 call) runs the images in chunks of B instead -- beyond the
reference, which loops image by image: per chunk one pinned staging buffer and one upload, one launch that resizes,
pads and stacks them all (``preprocess_batch``: mmdet's ``stack_batch`` shape), one forward, one launch for threshold
+ NMS + rescale of every image (``postprocess_batch``) and one download.  Every image's result is what the per-image
path returns for it when the model's detections do not depend on the other images of the batch.

``nms_type`` (beyond the reference, which runs hard NMS whatever the config says): ``None`` keeps the reference's
behaviour -- hard NMS at the config's ``iou_threshold``, ``max_per_img`` ignored.  ``"config"`` follows ``test_cfg[0]``
as mmdet does: ``nms.type`` ``'nms'`` is hard NMS, ``'soft_nms'`` is mmcv's soft-NMS with the config's ``method``
(default ``linear``), ``min_score`` (default 1e-3) and ``iou_threshold``; then the best ``max_per_img`` detections.
``"nms"`` / ``"soft_nms"`` force the mode with the other parameters still from the config.  In soft mode the returned
scores are the decayed ones, every call takes the chunked path and ``postprocess_batch`` is one
``hip_ops.postprocess_detections_soft`` launch per chunk; ``run_inference`` uses ``hip_ops.soft_nms``.

``tta`` (beyond the reference; mmdet's ``DetTTAModel`` + ``TestTimeAug``): ``None``, the default, changes nothing.  A dict
``dict(scales=[(long, short), ...], flip=bool, nms=dict(type='nms' | 'soft_nms', iou_threshold[, method, min_score]),
max_per_img=int | None)`` -- or ``"config"``, which reads ``cfg.tta_model['tta_cfg']`` and the ``Resize`` scales /
``RandomFlip`` probabilities of the ``TestTimeAug`` step of ``cfg.tta_pipeline`` -- runs every image as
``len(scales) * (2 if flip else 1)`` views and fuses their detections on the device.  View order:
``v = s * (2 if flip else 1) + f``, scales in the given order, the unflipped view of a scale before its flipped one.
Per chunk of ``batch_size`` images: one pinned staging copy and one upload (images, widths and every view's rescale
divisor); per scale one ``preprocess_views`` launch
(the chunk's images times the flips: keep-ratio resize to that scale, divisor padding, stacking -- no fixed-size ``Pad``
step, which mmdet's TTA pipelines do not have), one forward and one of the post-processing launches above with each
view's own scale factors as divisors; then one ``hip_ops.tta_merge`` launch and one download.  At most 16 views and
``views * num_queries <= 4096``.  Parity with mmdet / mmcv is unpinned (neither is installed here); as in the soft-NMS
kernel classes are told apart by comparing labels, ties go to the lowest index and the IoU arithmetic is the project's.

``tta["wbf"]`` (beyond the reference; weighted boxes fusion, Solovyev et al., as the ``ensemble_boxes`` package runs it):
``tta=dict(scales=..., flip=..., wbf=dict(iou_threshold=0.55, skip_box_thr=0.0, conf_type='avg' | 'max', weights=None),
max_per_img=...)`` merges the views with one ``hip_ops.wbf_merge`` launch in place of ``tta_merge``: the views' boxes are
clustered per class and every cluster comes back as its confidence-weighted mean box, with a score that says how many
views agreed; every prediction gains ``"votes"``, the number of boxes fused into each detection.  ``wbf`` and ``nms`` are
alternatives (both: ``ValueError``).  ``weights``: one per view, or one per model.  The rule, its two deviations from the
package (the tie rule; live = positive confidence) and its limits are stated in ``include/codetr_wbf.h``; parity with
``ensemble_boxes`` is unpinned (it is not installed here).

``ensemble`` (with ``tta`` only; beyond the reference): ``ensemble=[model_b, ...]`` names further models that run on the
same pre-processed views; their detections are further views of the merge, ``v = (k * S + s) * F + f`` with ``k = 0`` for
the main model, S scales and F flips.  All models must return the same number of detections per image; the 16-view and
4096-candidate limits apply to the total.  ``tta=dict(scales=[the config's scale], ...)`` is a plain ensemble.  It works
with the ``nms`` merges too.

``slicing`` (beyond the reference; sliced inference as in SAHI): ``None``, the default, changes nothing.  A dict
``dict(tile=(w, h), overlap=0.2 | (ox, oy), full_image=True, merge=dict(type='nmm' | 'nms', metric='ios' | 'iou',
threshold=0.5, class_agnostic=False), max_per_img=300, tile_batch=8)`` (the defaults shown; only ``tile`` is required)
cuts every image into overlapping tiles (``slice_grid``; y-major, then x; with ``full_image`` the whole image is the
last view), runs every tile as an image of its own -- the keep-ratio resize into the config's ``scale``, divisor
padding, no fixed-size ``Pad`` step, as a TTA view -- and fuses the views' detections on the device.  Per chunk of
``batch_size`` images: one pinned staging copy and one upload (the images, every view's origin and rescale divisor, the
image sizes and the view table), one ``preprocess_tiles`` launch per 32 rows (every row a crop of the uploaded image),
``ceil(rows / tile_batch)`` forwards each followed by the configured post-processing launch (hard, soft or none) with
the rows' own scale factors as divisors, then one ``hip_ops.slice_merge`` launch -- boxes shifted by the tile origin,
clipped to the image, greedy NMS or greedy non-maximum merging under IoU or IoS, cut to ``max_per_img`` -- and one
download.  At most 64 views per image and ``views * num_queries <= 4096``; not combined with ``tta``.  Parity with SAHI
is unpinned (it is not installed here): ties, label comparison and the overlap arithmetic are the project's, stated in
``include/codetr_hip.h``.

``visualizer`` (the reference builds mmdet's ``DetLocalVisualizer`` from ``cfg.visualizer``, :125-146, and draws in
``visualize``, :163-235): ``None``, the default, changes nothing.  A dict with any of ``line_width`` (1..15, default 3),
``alpha`` (0.8), ``text_color`` ((200, 200, 200)), ``font_scale`` (1..4), ``draw_labels``, ``palette`` and ``classes`` --
or ``"config"``, which reads ``line_width`` / ``alpha`` / ``text_color`` from ``cfg.visualizer`` and is a ``ValueError``
for a config without that entry -- turns the drawing on: ``__call__(..., return_vis=True)`` returns one ``[H, W, 3]``
uint8 array per image in ``results_dict["visualization"]``, and ``out_dir`` without ``no_save_vis`` writes
``out_dir/vis/%08d.png`` (PNG through stdlib ``zlib``, where the reference writes ``.jpg`` through cv2).
``vis_format="jpeg"`` or ``dict(type="jpeg", quality=90, subsampling="420" | "444")`` writes the reference's
``out_dir/vis/%08d.jpg`` instead: ``hip_ops.encode_jpeg`` encodes the chunk's images on the GPU where the drawing left
them (the file is stated in ``include/codetr_jpeg.h``) and only the compressed bytes come back -- the RGB buffer is
downloaded only when ``return_vis=True`` asks for the arrays; ``return_vis="jpeg"`` returns the files as ``bytes`` in
``results_dict["visualization_jpeg"]``.  ``vis_format=None`` (or ``"png"``), the default, changes nothing.
``pred_score_thr`` is the drawing's score threshold; ``draw_pred=False`` returns the original images.  Class names:
``visualizer["classes"]``, else ``dataset_meta["classes"]``, else ``str(label)``; cut to 23 characters, a non-ASCII
character becomes ``?``.  Palette: RGB triples from the same two places; for a name such as ``"coco"`` or nothing, a
generated table (``generated_palette``: mmdet's named palettes are not part of this build).  A visualising call takes
the chunked path; per chunk one ``hip_ops.draw_detections`` launch draws every image's final detections (plain, soft
the TTA merge's or the slice merge's, cut to ``max_per_img``) on the buffer the chunk's one upload filled, in place and after the last
preprocessing launch on the stream, and one more device-to-host copy fetches that buffer.  The rendering is the
project's own, modelled on ``DetLocalVisualizer``'s defaults and stated pixel by pixel in ``include/codetr_hip.h``.
Parity with mmdet's visualiser is unpinned (neither mmdet nor matplotlib is installed here).

``input_format`` / ``color`` of ``__call__`` (beyond the reference, which takes host RGB arrays): ``"rgb"``, the default,
with numpy arrays changes nothing.  ``"bgr"``, ``"rgba"``, ``"bgra"``, ``"gray"``, ``"nv12"``, ``"nv21"`` and ``"i420"``
take frames as decoders and capture libraries hand them out -- numpy arrays or ``torch.uint8`` tensors, on the host or
already on the GPU; for the YUV formats the 2-D ``[H * 3 / 2, W]`` array or a tuple of planes (``parse_frame``).
``color`` = ``dict(matrix='bt601' | 'bt709', range='limited' | 'full')``, default BT.601 limited, is the YUV matrix.
Such a call takes the chunked path; per chunk ``stage_chunk`` uploads the raw planes (1.5 bytes per pixel of NV12 /
I420 instead of 3) in the one pinned staging copy and one ``hip_ops.frames_to_rgb`` launch writes them as the packed
RGB buffer every other kernel reads; GPU-resident frames -- pitched views of a decoder surface among them -- are not
uploaded at all: one launch per group of frames that share a storage reads them where they lie.  The visualisation draws
on, and returns, the converted RGB frames.  The conversion is stated in integer arithmetic in ``include/codetr_hip.h``;
parity with OpenCV's ``cvtColor`` is unpinned (cv2 is not installed here).

``tracker`` (beyond the reference; tracking-by-detection modelled on mmdet's ``ByteTracker``): ``None``, the default,
changes nothing -- no new key, no new launch, the per-image route as it is.  A dict with any of the keys of
``hip_ops.TRACKER`` (``obj_score_thrs``, ``init_track_thr``, ``weight_iou_with_det_scores``, ``match_iou_thrs``,
``num_frames_retain``, ``num_tentatives``, ``max_tracks``) -- or ``"config"``, which reads a ``tracker`` entry of the config
-- turns it on: every result dict gains ``"track_ids"``, one int per detection: the id of its track, negated while the
track is tentative, 0 for none.  ``__call__(..., streams=...)`` names the stream (camera) of every frame, one
non-negative int or one per frame, default 0; the frames of a stream are in temporal order within and across calls, a
stream's state is created on its first frame and ``reset_tracks(stream=None)`` zeroes one or all.  A tracked call takes
the chunked path; after the chunk's final detections one ``hip_ops.track_update`` launch (one workgroup per stream, the
stream's frames walked in order) and one more device-to-host copy of ``[N, Q]`` int32; the states stay on the device.
The ids are cut as the detections are, the hard path's host-side ``max_per_img`` cut included (the tracker itself
sees every row of the launch's result).  The rule is stated in
``include/codetr_hip.h``; parity with mmdet is unpinned (it is not installed here): the association is greedy, labels
are compared and ties go to the lowest slot and row.

``track_association`` (with a tracker only): ``None``, the default, or ``"greedy"`` keeps that rule and its launch;
``"optimal"`` makes each of the three associations an assignment problem over integer gains, as mmdet's ``lapjv`` call
does, solved inside the same one launch per chunk (``include/codetr_assign.h`` states the gains, the procedure and its
tie rule; ``csrc/track_common.h``).  Greedy loses an identity where two objects cross and the best single pair leaves
the other track nothing above the threshold; the assignment keeps both.  The states are the same for both rules.

``track_motion`` (with a tracker only): ``None``, the default, changes nothing.  ``"translation"`` or
``dict(type="translation", grid=160, search=8, texture=2, min_blocks=4)`` turns camera-motion compensation on: per chunk
``hip_ops.estimate_motion`` (three launches behind the staging, in front of the forward and of the drawing;
``csrc/motion.hip``) estimates the translation between the consecutive frames of every stream from the chunk's own
images, the motion stays on the device and ``codetr_track_update3_*`` adds it to the predicted track centres before
association, so a pan, a shake or a preset change keeps the ids.  Every result dict gains ``"camera_motion"``:
``[dx, dy]`` in source pixels, or ``None`` where there is none (a stream's first frame, a size change, too little texture
or agreement).  ``include/codetr_motion.h`` states the rule and its limits: translation only, a reach of ``search * k``
pixels per frame (96 px at 1920 x 1080 by default).

``"similarity"`` (same keys) fits a zoom and a roll as well as the pan to the same block votes (two more launches, the
header's version 2) and ``codetr_track_update4_*`` moves the predicted centres, their velocities and the heights with it: a
PTZ camera that zooms, a drone that climbs or yaws, a handheld camera that rolls.  A frame whose similarity is not valid
falls back to its translation, so the mode is never worse than ``"translation"``.  ``"camera_motion"`` stays ``[dx, dy]`` (of
a similarity: the inliers' mean displacement), and every result dict also gains ``"camera_transform"``: the 2 x 3 matrix
``[[a, -b, tx], [b, a, ty]]`` that maps a point of the stream's previous frame to this one (``[[1, 0, dx], [0, 1, dy]]``
for a translation), or ``None``.  Shear and perspective are not modelled and the boxes stay axis-aligned.

``track_appearance`` (with a tracker only): ``None``, the default, means no launch and no change.  ``"color"`` or
``dict(type="color", appearance_thr=0.75, proximity_thr=0.5, reid_gate=1.5)`` adds an appearance cue to the first two
associations: per chunk, after the chunk's final detections and before the drawing launch writes into the RGB buffer, one
``hip_ops.appearance_descriptors`` launch (``csrc/appearance.hip``) gathers a colour histogram of every detection from the
chunk's own images, and ``codetr_track_update5_*`` adds its similarity with the track's kept appearance to the pair value:
an object that re-enters away from its prediction keeps its id, and two objects that change lanes behind an occluder do
not swap theirs.  It works with every ``input_format``, ``track_association`` and ``track_motion``; predictions gain no
key.  ``include/codetr_appearance.h`` states the rule and its limits: hard 2-bit colour bins, two stripes, nothing learned.

``redact``: ``None``, the default, means no launch, no new key and no change.
``dict(mode="pixelate", classes=None, score_thr=0.3, expand=0.1, shape="box", cell=16, fill=(0, 0, 0))`` (``redact_settings``)
makes the detected regions unrecognisable in every image that leaves the call: per chunk, after ``track_chunk`` (the
appearance descriptors read the original pixels) and before the drawing and the JPEG encoder, ``hip_ops.redact_detections``
(``csrc/redact.hip``) pixelates, blurs or fills, in place in the chunk's RGB buffer, the box -- grown by ``expand``, or the
ellipse inside it -- of every final detection of the selected classes with a score above ``score_thr``.  With ``redact``
set, ``return_vis`` and ``out_dir`` work without a visualiser and give the redacted images undrawn; with one the outlines
and labels are drawn over the redacted pixels; ``draw_pred=False`` gives redaction without drawing; a JPEG ``vis_format``
encodes the redacted buffer.  Every result dict gains ``"redacted"``: the indices of its rows that were selected.
``include/codetr_redact.h`` states the rule byte for byte; "blur" is the library's own (cell means and a tent), parity with
OpenCV's blur is unpinned.
"""
import collections
import colorsys
import json
import os
import struct
import zlib
from typing import Dict, List, Optional

import numpy as np
import torch

from . import hip_ops
from .config import Config


def rescale_size(h, w, scale):
    """mmcv.imrescale: (new_h, new_w) for a keep-ratio resize into the (long, short) bound pair `scale`"""
    f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(h * f + 0.5), int(w * f + 0.5)


def nms_settings(test_cfg, nms_type=None):
    """How `Inferencer(..., nms_type=...)` reads the query head's test_cfg (mmdet: `batched_nms(.., test_cfg.nms)` then
    `[:max_per_img]`): -> dict(type 'nms' | 'soft_nms', method, min_score, max_per_img or None).  nms_type None is the
    reference's simplification: hard NMS and no cut, whatever the config says."""
    if nms_type not in (None, "config", "nms", "soft_nms"):
        raise ValueError(f"nms_type must be None, 'config', 'nms' or 'soft_nms', got {nms_type!r}")
    nms_cfg = dict(test_cfg["nms"]) if "nms" in test_cfg else {}
    out = dict(type="nms", method=nms_cfg.get("method", "linear"), min_score=float(nms_cfg.get("min_score", 1e-3)),
               max_per_img=None, forced_without_entry=False)   # (mmcv's soft_nms defaults: linear, 1e-3)
    if nms_type is None:
        return out
    out["type"] = nms_cfg.get("type", "nms") if nms_type == "config" else nms_type
    if out["type"] not in ("nms", "soft_nms"):
        raise NotImplementedError(f"nms type {out['type']!r}: 'nms' and 'soft_nms' are built")
    if "nms" not in test_cfg:
        if nms_type == "config":
            raise NotImplementedError("test_cfg[0] without an nms entry: only the NMS forms of mmdet's post-processing "
                                      "are built")
        out["forced_without_entry"] = True
    if test_cfg.get("max_per_img", -1) > 0:
        out["max_per_img"] = int(test_cfg["max_per_img"])
    if out["type"] == "soft_nms":
        hip_ops._soft_method(out["method"])   # 'gaussian' raises NotImplementedError, an unknown name ValueError
    return out



def _pairs(scale):
    """a Resize `scale` (one (long, short) pair, or a list of them) -> list of pairs"""
    if len(scale) == 2 and all(isinstance(v, (int, float)) for v in scale):
        return [tuple(int(v) for v in scale)]
    return [tuple(int(v) for v in pair) for pair in scale]


def tta_settings(cfg, tta):
    """How `Inferencer(..., tta=...)` reads its argument: None -> None; a dict(scales, flip, nms | wbf, max_per_img) is
    validated (`wbf`: the dict of hip_ops.wbf_settings -- weighted boxes fusion in place of the NMS merge; the result
    then holds it completed under "wbf" and None under "nms", otherwise None under "wbf"); "config" takes `cfg.tta_model['tta_cfg']` (nms, max_per_img) and, from the TestTimeAug step of
    `cfg.tta_pipeline`, every Resize scale and whether the RandomFlip branch holds both prob 0 and prob 1 (ValueError
    when the config has neither entry).  -> dict(scales [(long, short)], flip, nms dict(type, iou_threshold, method,
    min_score), max_per_img or None, views [(scale, flipped)] in launch order: v = s * (2 if flip else 1) + f,
    unflipped first)."""
    if tta is None:
        return None
    if tta == "config":
        model, pipeline = cfg.get("tta_model"), cfg.get("tta_pipeline")
        if model is None or pipeline is None:
            raise ValueError("tta='config': the config has no tta_model / tta_pipeline")
        tta_cfg = dict(model.get("tta_cfg", {}))
        steps = [s for s in pipeline if s.get("type") == "TestTimeAug"]
        if len(steps) != 1:
            raise ValueError("tta='config': tta_pipeline needs exactly one TestTimeAug step")
        scales, probs = [], []
        for branch in steps[0]["transforms"]:
            for t in branch:
                if t.get("type") == "Resize":
                    if not t.get("keep_ratio", False):
                        raise NotImplementedError("TTA views are keep_ratio=True resizes")
                    scales += _pairs(t["scale"])
                elif t.get("type") == "RandomFlip":
                    if t.get("direction", "horizontal") != "horizontal":
                        raise NotImplementedError("only the horizontal flip is built")
                    probs.append(float(t.get("prob", 0.0)))
        if any(p not in (0.0, 1.0) for p in probs) or (probs and 0.0 not in probs):
            raise NotImplementedError(f"RandomFlip probabilities {probs}: a TTA flip branch is prob=0. [and prob=1.]")
        tta = dict(scales=scales, flip=1.0 in probs, nms=tta_cfg.get("nms", dict(type="nms", iou_threshold=0.5)),
                   max_per_img=tta_cfg.get("max_per_img"))
    if not isinstance(tta, dict) or set(tta) - {"scales", "flip", "nms", "wbf", "max_per_img"} or "scales" not in tta:
        raise ValueError("tta must be None, 'config' or dict(scales, flip, nms | wbf, max_per_img)")
    if tta.get("wbf") is not None and tta.get("nms") is not None:
        raise ValueError("tta: nms and wbf are two ways to merge the views: give one of them")
    scales = _pairs(tta["scales"]) if tta["scales"] else []
    if not scales or any(len(p) != 2 or min(p) <= 0 for p in scales):
        raise ValueError("tta scales: a non-empty list of positive (long, short) pairs")
    flip = bool(tta.get("flip", False))
    nms = dict(tta.get("nms") or dict(type="nms", iou_threshold=0.5))
    kind = nms.get("type", "nms")
    if kind not in ("nms", "soft_nms"):
        raise NotImplementedError(f"tta nms type {kind!r}: 'nms' and 'soft_nms' are built"
                                  + (" (weighted boxes fusion is the tta key wbf=dict(...))" if kind == "wbf" else ""))
    out_nms = dict(type=kind, iou_threshold=float(nms.get("iou_threshold", 0.5 if kind == "nms" else 0.3)),
                   method=nms.get("method", "linear"), min_score=float(nms.get("min_score", 1e-3)))
    if kind == "soft_nms":
        hip_ops._soft_method(out_nms["method"])   # 'gaussian' raises NotImplementedError, an unknown name ValueError
    mpi = tta.get("max_per_img")
    views = [(s, f) for s in scales for f in ((False, True) if flip else (False,))]
    if len(views) > hip_ops.TTA_MAX_VIEWS:
        raise ValueError(f"tta: {len(views)} views, at most {hip_ops.TTA_MAX_VIEWS} (scales x flips) are merged")
    wbf = hip_ops.wbf_settings(tta["wbf"]) if tta.get("wbf") is not None else None
    return dict(scales=scales, flip=flip, nms=out_nms if wbf is None else None, wbf=wbf,
                max_per_img=int(mpi) if mpi is not None and mpi > 0 else None, views=views)


def ensemble_settings(ensemble, tta):
    """How `Inferencer(..., ensemble=...)` reads its argument: None (or an empty list) -> []; a list of further models,
    which run on the views of `tta` (the result of tta_settings) next to the main model, their detections further views
    of the merge: v = (k * S + s) * F + f with k = 0 for the main model.  ValueError without tta, for more views in all
    than the merge takes, and for wbf weights that are neither one per view nor one per model; per-model weights are
    expanded to per-view weights in tta["wbf"]."""
    models = list(ensemble) if ensemble is not None else []
    if models and tta is None:
        raise ValueError("ensemble needs tta: tta=dict(scales=[the config's scale], ...) is a plain ensemble")
    if tta is None:
        return models
    per_model, total = len(tta["views"]), len(tta["views"]) * (1 + len(models))
    if total > hip_ops.TTA_MAX_VIEWS:
        raise ValueError(f"ensemble: {1 + len(models)} models x {per_model} views, at most {hip_ops.TTA_MAX_VIEWS} views "
                         "are merged")
    w = tta["wbf"]["weights"] if tta["wbf"] is not None else None
    if w is not None:
        if len(w) == 1 + len(models):
            tta["wbf"]["weights"] = [wk for wk in w for _ in range(per_model)]
        elif len(w) != total:
            raise ValueError(f"wbf weights: {len(w)} given, one per view ({total}) or one per model ({1 + len(models)})")
    return models


SLICING_KEYS = ("tile", "overlap", "full_image", "merge", "max_per_img", "tile_batch")


def slicing_settings(slicing):
    """How `Inferencer(..., slicing=...)` reads its argument: None -> None; a dict with keys of SLICING_KEYS is
    validated and completed -> dict(tile (w, h), overlap (ox, oy), full_image, merge (hip_ops.slice_merge_settings),
    max_per_img or None, tile_batch)."""
    if slicing is None:
        return None
    if not isinstance(slicing, dict) or set(slicing) - set(SLICING_KEYS) or "tile" not in slicing:
        raise ValueError(f"slicing must be None or a dict with 'tile' and keys of {SLICING_KEYS}")
    tile = tuple(slicing["tile"])
    if len(tile) != 2 or any(int(t) != t or t < 1 for t in tile):
        raise ValueError("slicing tile: (width, height), positive integers")
    overlap = slicing.get("overlap", 0.2)
    overlap = tuple(overlap) if isinstance(overlap, (tuple, list)) else (overlap, overlap)
    if len(overlap) != 2 or any(not 0 <= float(o) < 1 for o in overlap):
        raise ValueError("slicing overlap: a ratio, or (ox, oy), each in [0, 1)")
    mpi = slicing.get("max_per_img", 300)
    tile_batch = slicing.get("tile_batch", 8)
    if int(tile_batch) != tile_batch or tile_batch < 1:
        raise ValueError(f"slicing tile_batch must be a positive integer, got {tile_batch}")
    return dict(tile=(int(tile[0]), int(tile[1])), overlap=(float(overlap[0]), float(overlap[1])),
                full_image=bool(slicing.get("full_image", True)), merge=hip_ops.slice_merge_settings(slicing.get("merge")),
                max_per_img=int(mpi) if mpi is not None and mpi > 0 else None, tile_batch=int(tile_batch))


def tracker_settings(tracker, cfg=None):
    """How `Inferencer(..., tracker=...)` reads its argument: None -> None; a dict with keys of hip_ops.TRACKER is
    validated and completed from it (hip_ops.track_settings: ValueError for an unknown key or a value out of range);
    "config" takes the `tracker` entry of the config `cfg` (its `type` key dropped; ValueError when the config has
    none)."""
    if tracker is None:
        return None
    if isinstance(tracker, str):
        entry = cfg.get("tracker") if tracker == "config" and cfg is not None else None
        if entry is None:
            raise ValueError("tracker='config': the config has no tracker entry" if tracker == "config"
                             else f"tracker must be None, 'config' or a dict, got {tracker!r}")
        tracker = {k: v for k, v in dict(entry).items() if k != "type"}
    if not isinstance(tracker, dict):
        raise ValueError(f"tracker must be None, 'config' or a dict with keys of {sorted(hip_ops.TRACKER)}")
    return hip_ops.track_settings(tracker)


FRAME_COLOR_KEYS = ("matrix", "range")


def frame_settings(input_format="rgb", color=None):
    """How `__call__(..., input_format=..., color=...)` reads its arguments: `input_format` a name of
    hip_ops.FRAME_FORMATS ('rgb', 'bgr', 'rgba', 'bgra', 'gray', 'nv12', 'nv21', 'i420'); `color` None or a dict with any
    of `matrix` ('bt601' | 'bt709') and `range` ('limited' | 'full'), completed from hip_ops.FRAME_COLOR (BT.601,
    limited range: what OpenCV's cvtColor computes) -- only the YUV formats read it.  `input_format` may also be 'jpeg':
    the items are baseline JPEG files (bytes, 1-D uint8 arrays or paths), decoded on the GPU (`hip_ops.decode_jpeg`).
    -> dict(format, matrix, range)"""
    if input_format != "jpeg" and (not isinstance(input_format, str) or input_format not in hip_ops.FRAME_FORMATS):
        raise ValueError(f"input_format must be one of {sorted(hip_ops.FRAME_FORMATS)}, got {input_format!r}")
    if color is not None and (not isinstance(color, dict) or set(color) - set(FRAME_COLOR_KEYS)):
        raise ValueError(f"color must be None or a dict with keys of {FRAME_COLOR_KEYS}, got {color!r}")
    out = dict(hip_ops.FRAME_COLOR, **(color or {}))
    if out["matrix"] not in ("bt601", "bt709"):
        raise ValueError(f"color matrix must be 'bt601' or 'bt709', got {out['matrix']!r}")
    if out["range"] not in ("limited", "full"):
        raise ValueError(f"color range must be 'limited' or 'full', got {out['range']!r}")
    return dict(format=input_format, matrix=out["matrix"], range=out["range"])


# one frame of a chunk: the format's code, its size, its planes as 2-D byte arrays [rows, row bytes] -- numpy on the host,
# torch tensors with strides (pitch, 1) on the GPU -- and whether they are on the GPU
Frame = collections.namedtuple("Frame", "code H W planes resident")

_FRAME_SHAPES = dict(rgb="(H, W, 3)", bgr="(H, W, 3)", rgba="(H, W, 4)", bgra="(H, W, 4)", gray="(H, W)",
                     nv12="(H * 3 / 2, W) with even H and W, or planes (y (H, W), uv (ceil(H / 2), ceil(W / 2), 2))",
                     nv21="(H * 3 / 2, W) with even H and W, or planes (y (H, W), vu (ceil(H / 2), ceil(W / 2), 2))",
                     i420="(H * 3 / 2, W) with even H and W, or planes (y (H, W), u, v (ceil(H / 2), ceil(W / 2)))")


def parse_frame(item, input_format="rgb"):
    """One chunk item -> Frame.  `item`: a numpy array or a torch tensor, uint8, on the host or on the GPU, of the
    format's shape (_FRAME_SHAPES); for nv12 / nv21 / i420 either the 2-D array decoders hand out or a tuple of planes.
    A host plane may have any strides (it is copied row by row into the staging buffer); a GPU-resident plane is read
    where it lies and needs unit innermost stride and a positive row stride of at least the row's bytes, which becomes
    its pitch -- a crop of a wider surface, say.  Anything else is a ValueError that names the format."""
    fmt = input_format

    def bad(why):
        return ValueError(f"input_format={fmt!r}: expected uint8 frames of shape {_FRAME_SHAPES[fmt]}; {why}")

    def array(a):
        if torch.is_tensor(a):
            if a.dtype != torch.uint8:
                raise bad(f"got a tensor of {a.dtype}")
            return a if a.is_cuda else a.detach().numpy()
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
            raise bad(f"got {type(a).__name__}" + (f" of {a.dtype}" if isinstance(a, np.ndarray) else ""))
        return a

    def rows2d(a):
        """[R, W] or [R, W, C] -> the byte rows [R, W * C]"""
        R, B = a.shape[0], int(np.prod(a.shape[1:]))
        if isinstance(a, np.ndarray):
            return a.reshape(R, B)          # (a copy where the strides do not allow a view: host planes are copied anyway)
        inner, unit = [], 1
        for size, stride in zip(reversed(a.shape[1:]), reversed(a.stride()[1:])):
            inner.append(size == 1 or stride == unit)
            unit *= size
        if not all(inner) or (R > 1 and a.stride(0) < B):
            raise bad(f"a GPU-resident plane needs unit innermost stride and a row stride of at least the row's bytes, "
                      f"got strides {tuple(a.stride())} for shape {tuple(a.shape)}")
        return a.as_strided((R, B), (a.stride(0) if R > 1 else B, 1))

    if isinstance(item, (tuple, list)):
        if fmt not in ("nv12", "nv21", "i420"):
            raise bad("got a tuple of planes")
        parts = [array(a) for a in item]
        if len(parts) != (3 if fmt == "i420" else 2) or parts[0].ndim != 2 or min(parts[0].shape) < 1:
            raise bad(f"got {len(parts)} plane(s)" + (f", y of shape {tuple(parts[0].shape)}" if parts else ""))
        H, W = (int(v) for v in parts[0].shape)
        chroma = ((H + 1) // 2, (W + 1) // 2) + ((2,) if fmt != "i420" else ())
        for a in parts[1:]:
            if tuple(a.shape) != chroma:
                raise bad(f"got a chroma plane of shape {tuple(a.shape)} for a {H} x {W} frame, expected {chroma}")
        planes = [rows2d(a) for a in parts]
    else:
        a = array(item)
        if fmt in ("nv12", "nv21", "i420"):
            if a.ndim != 2 or a.shape[0] % 3 or (a.shape[0] * 2 // 3) % 2 or a.shape[1] % 2 or min(a.shape) < 1:
                raise bad(f"got shape {tuple(a.shape)}")
            H, W = int(a.shape[0]) * 2 // 3, int(a.shape[1])
            if fmt != "i420":
                planes = [rows2d(a[:H]), rows2d(a[H:])]
            else:   # two chroma rows lie in every row of the lower third: only an unpitched array splits into planes
                if isinstance(a, np.ndarray):
                    c = np.ascontiguousarray(a[H:])
                elif a.stride(1) == 1 and a.stride(0) == W:
                    c = a[H:]
                else:
                    raise bad(f"a GPU-resident 2-D i420 frame must be contiguous (strides {tuple(a.stride())}): pass the "
                              "planes (y, u, v) of a pitched surface")
                c = c.reshape(2, H // 2, W // 2)
                planes = [rows2d(a[:H]), rows2d(c[0]), rows2d(c[1])]
        else:
            C = dict(rgb=3, bgr=3, rgba=4, bgra=4, gray=0)[fmt]
            if a.ndim != (3 if C else 2) or (C and a.shape[2] != C) or min(a.shape) < 1:
                raise bad(f"got shape {tuple(a.shape)}")
            H, W = int(a.shape[0]), int(a.shape[1])
            planes = [rows2d(a)]
    on_gpu = [torch.is_tensor(p) for p in planes]
    if any(on_gpu):
        if not all(on_gpu) or len({p.untyped_storage().data_ptr() for p in planes}) != 1:
            raise bad("the planes of a GPU-resident frame must share one storage (views of one surface)")
    return Frame(hip_ops.FRAME_FORMATS[fmt], H, W, planes, all(on_gpu))


def generated_palette(n):
    """n RGB triples for classes without a palette of their own: the hue steps by the golden ratio (neighbouring
    labels get distant colours), fixed saturation and value; the same table on every call"""
    out = []
    for i in range(n):
        r, g, b = colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, 0.75, 1.0)
        out.append((int(r * 255 + 0.5), int(g * 255 + 0.5), int(b * 255 + 0.5)))
    return out


VISUALIZER_KEYS = ("line_width", "alpha", "text_color", "font_scale", "draw_labels", "palette", "classes")


def _meta(dataset_meta, key):
    if dataset_meta is None:
        return None
    return dataset_meta.get(key) if isinstance(dataset_meta, dict) else getattr(dataset_meta, key, None)


def visualizer_settings(cfg, visualizer, dataset_meta=None):
    """How `Inferencer(..., visualizer=...)` reads its argument: None -> None; a dict with keys of VISUALIZER_KEYS (the
    style of hip_ops.draw_detections without score_thr, which is the call's pred_score_thr, plus `palette` and
    `classes`) is validated; "config" takes line_width / alpha / text_color from `cfg.visualizer` (ValueError when the
    config has no such entry, the case in which the reference raises).  Class names: visualizer['classes'], else
    dataset_meta['classes'], else str(label) for the query head's num_classes labels.  Palette: a list of RGB triples
    from the same two places; for a name such as 'coco', or nothing, `generated_palette`.
    -> dict(style, classes [str], palette [(r, g, b)], names: the [C, 24] uint8 table, colors: [C, 3] uint8)"""
    if visualizer is None:
        return None
    if visualizer == "config":
        entry = cfg.get("visualizer")
        if entry is None:
            raise ValueError('visualizer="config": the config has no "visualizer" entry')
        visualizer = {k: entry[k] for k in ("line_width", "alpha", "text_color") if k in entry}
    if not isinstance(visualizer, dict):
        raise ValueError(f"visualizer must be None, 'config' or a dict with keys of {VISUALIZER_KEYS}")
    unknown = set(visualizer) - set(VISUALIZER_KEYS)
    if unknown:
        raise ValueError(f"visualizer: unknown key(s) {sorted(unknown)}; known: {list(VISUALIZER_KEYS)}")
    style = hip_ops.draw_style({k: v for k, v in visualizer.items() if k not in ("palette", "classes")})
    classes = visualizer.get("classes")
    if classes is None:
        classes = _meta(dataset_meta, "classes")
    if classes is None:
        head = cfg.model.get("query_head") or {}
        classes = [str(i) for i in range(int(head.get("num_classes", 80)))]
    classes = [str(c) for c in classes]
    if not classes:
        raise ValueError("visualizer: no classes")
    palette = visualizer.get("palette")
    if palette is None:
        palette = _meta(dataset_meta, "palette")
    if palette is None or isinstance(palette, str):
        palette = generated_palette(len(classes))   # (mmdet's named palettes are not part of this build)
    palette = [tuple(int(v) for v in c) for c in palette]
    if len(palette) != len(classes) or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in palette):
        raise ValueError("visualizer: the palette needs one RGB triple in 0..255 per class")
    return dict(style=style, classes=classes, palette=palette, names=hip_ops.draw_names_table(classes),
                colors=torch.tensor(palette, dtype=torch.uint8).view(-1, 3))


REDACT_KEYS = ("mode", "classes", "score_thr", "expand", "shape", "cell", "fill")


def redact_settings(cfg, redact, dataset_meta=None, visualizer=None):
    """How `Inferencer(..., redact=...)` reads its argument: None -> None; a dict with keys of REDACT_KEYS is validated
    and completed from hip_ops.REDACT (hip_ops.redact_style: a ValueError names the key) plus `classes`: None (every
    label) or a list of class names or ids.  Names resolve as the visualiser's do: `visualizer['classes']` (the settings
    visualizer_settings returned), else dataset_meta['classes'], else str(label) for the query head's num_classes labels.
    -> dict(style, classes: the sorted ids or None, select: the [C] uint8 table of hip_ops.redact_detections or None)"""
    if redact is None:
        return None
    if not isinstance(redact, dict):
        raise ValueError(f"redact must be None or a dict with keys of {REDACT_KEYS}")
    unknown = set(redact) - set(REDACT_KEYS)
    if unknown:
        raise ValueError(f"redact: unknown key(s) {sorted(unknown)}; known: {list(REDACT_KEYS)}")
    style = hip_ops.redact_style({k: v for k, v in redact.items() if k != "classes"})
    classes = redact.get("classes")
    if classes is None:
        return dict(style=style, classes=None, select=None)
    names = visualizer["classes"] if visualizer is not None else _meta(dataset_meta, "classes")
    if names is None:
        head = cfg.model.get("query_head") or {}
        names = [str(i) for i in range(int(head.get("num_classes", 80)))]
    names = [str(c) for c in names]
    if isinstance(classes, (str, bytes)) or not isinstance(classes, (list, tuple)) or len(classes) == 0:
        raise ValueError(f"redact: classes must be None or a non-empty list of class names or ids, got {classes!r}")
    ids = set()
    for c in classes:
        if isinstance(c, str):
            if c not in names:
                raise ValueError(f"redact: classes: unknown class name {c!r}")
            ids.add(names.index(c))
        elif isinstance(c, (int, np.integer)) and not isinstance(c, bool) and 0 <= int(c) < len(names):
            ids.add(int(c))
        else:
            raise ValueError(f"redact: classes: {c!r} is neither a class name nor an id in 0..{len(names) - 1}")
    select = torch.zeros(len(names), dtype=torch.uint8)
    select[sorted(ids)] = 1
    return dict(style=style, classes=sorted(ids), select=select)


def redacted_rows(pred, redact):
    """the indices of the rows of a prediction dict that the redaction selects (include/codetr_redact.h, "Selection"),
    from the labels, scores and boxes the prediction carries: score > score_thr in fp32, a selected label, four finite
    coordinates"""
    thr = np.float32(redact["style"]["score_thr"])
    chosen = None if redact["classes"] is None else set(redact["classes"])
    boxes = np.asarray(pred["bboxes"], np.float32).reshape(-1, 4)
    return [j for j, (s, l) in enumerate(zip(pred["scores"], pred["labels"]))
            if np.float32(s) > thr and (chosen is None or l in chosen) and bool(np.isfinite(boxes[j]).all())]


VIS_FORMAT_KEYS = ("type", "quality", "subsampling")
VIS_DOWNLOADS = {"rgb": 0}   # device-to-host copies of a chunk's whole RGB buffer made for the visualisation, this process


def track_association_setting(track_association, tracker):
    """How `Inferencer(..., track_association=...)` reads its argument: None -> "greedy"; a name of
    hip_ops.TRACK_ASSOCIATIONS; ValueError for anything else, and for a name given without a tracker"""
    if track_association is None:
        return "greedy"
    if not isinstance(track_association, str) or track_association not in hip_ops.TRACK_ASSOCIATIONS:
        raise ValueError(f"track_association must be None or one of {list(hip_ops.TRACK_ASSOCIATIONS)}, "
                         f"got {track_association!r}")
    if tracker is None:
        raise ValueError("track_association without a tracker: Inferencer(..., tracker=dict(...)) turns tracking on")
    return track_association


def track_motion_model(track_motion):
    """the model of a `track_motion` argument that track_motion_settings accepted: None, "translation" or
    "similarity" (a string, or a dict's type)"""
    if track_motion is None:
        return None
    return track_motion if isinstance(track_motion, str) else track_motion["type"]


def camera_transform(row):
    """a row of hip_ops.estimate_motion(model="similarity") (dx, dy, valid, model, a, b, px, py) -> the 2 x 3 matrix
    [[a, -b, tx], [b, a, ty]] as nested lists, t = (px + dx, py + dy) - M (px, py), in float64 from the eight floats;
    [[1, 0, dx], [0, 1, dy]] for a translation row; None for an invalid one"""
    dx, dy, valid, model, a, b, px, py = (float(v) for v in row)
    if valid != 1.0:
        return None
    if model != 2.0:
        return [[1.0, 0.0, dx], [0.0, 1.0, dy]]
    return [[a, -b, (px + dx) - (a * px - b * py)], [b, a, (py + dy) - (b * px + a * py)]]


def track_motion_settings(track_motion, tracker):
    """How `Inferencer(..., track_motion=...)` reads its argument: None -> None; "translation" or "similarity" (the model:
    track_motion_model) -> hip_ops.MOTION;
    dict(type="translation", grid=..., search=..., texture=..., min_blocks=...) is validated and completed from it
    (hip_ops.motion_settings); ValueError for anything else, and for a setting given without a tracker"""
    if track_motion is None:
        return None
    if isinstance(track_motion, str):
        track_motion = dict(type=track_motion)
    if not isinstance(track_motion, dict) or track_motion.get("type") not in hip_ops.MOTION_MODELS:
        raise ValueError('track_motion must be None, "translation", "similarity" or a dict with one of them as type and keys of '
                         f"{sorted(hip_ops.MOTION)}, got {track_motion!r}")
    if tracker is None:
        raise ValueError("track_motion without a tracker: Inferencer(..., tracker=dict(...)) turns tracking on")
    return hip_ops.motion_settings({k: v for k, v in track_motion.items() if k != "type"})


def track_appearance_settings(track_appearance, tracker):
    """How `Inferencer(..., track_appearance=...)` reads its argument: None -> None; "color" -> hip_ops.APPEARANCE; a dict
    with type="color" and keys of hip_ops.APPEARANCE is validated and completed from it (hip_ops.appearance_settings);
    ValueError for anything else, and for a setting given without a tracker"""
    if track_appearance is None:
        return None
    if isinstance(track_appearance, str):
        track_appearance = dict(type=track_appearance)
    if not isinstance(track_appearance, dict) or track_appearance.get("type") != "color":
        raise ValueError('track_appearance must be None, "color" or a dict with type="color" and keys of '
                         f"{sorted(hip_ops.APPEARANCE)}, got {track_appearance!r}")
    if tracker is None:
        raise ValueError("track_appearance without a tracker: Inferencer(..., tracker=dict(...)) turns tracking on")
    return hip_ops.appearance_settings({k: v for k, v in track_appearance.items() if k != "type"})


def vis_format_settings(vis_format):
    """How `Inferencer(..., vis_format=...)` reads its argument: None and "png" -> None (vis/%08d.png through zlib, as
    before); "jpeg" or a dict with keys of VIS_FORMAT_KEYS, type "jpeg" -> dict(quality, subsampling), the validated
    settings of hip_ops.encode_jpeg (vis/%08d.jpg, the reference's name, encoded on the GPU).  ValueError otherwise."""
    if vis_format is None or vis_format == "png":
        return None
    if vis_format == "jpeg":
        vis_format = dict(type="jpeg")
    if not isinstance(vis_format, dict):
        raise ValueError(f"vis_format must be None, 'png', 'jpeg' or a dict with keys of {VIS_FORMAT_KEYS}")
    unknown = set(vis_format) - set(VIS_FORMAT_KEYS)
    if unknown:
        raise ValueError(f"vis_format: unknown key(s) {sorted(unknown)}; known: {list(VIS_FORMAT_KEYS)}")
    kind = vis_format.get("type", "jpeg")
    if kind == "png":
        if len(vis_format) > 1:
            raise ValueError("vis_format: type 'png' takes no settings")
        return None
    if kind != "jpeg":
        raise ValueError(f"vis_format: type must be 'png' or 'jpeg', got {kind!r}")
    return hip_ops.jpeg_settings({k: v for k, v in vis_format.items() if k != "type"})


def write_png(path, image):
    """an RGB uint8 image [H, W, 3] as an 8-bit truecolour PNG: filter 0 on every row, one IDAT at a low zlib level"""
    image = np.ascontiguousarray(image, np.uint8)
    H, W = image.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)
    rows[:, 1:] = image.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + chunk(b"IEND", b""))


class Inferencer:
    def __init__(self, model, model_file: str, dataset_meta, score_threshold: Optional[float] = None,
                 iou_threshold: Optional[float] = None, nms_type: Optional[str] = None, tta=None, visualizer=None,
                 slicing=None, tracker=None, vis_format=None,
                 track_association=None, ensemble=None, track_motion=None, track_appearance=None, redact=None):
        self.model = model
        self.dataset_meta = dataset_meta
        self.cfg = Config.fromfile(model_file)
        test_cfg = self.cfg.model.test_cfg[0]  # the 0th test_cfg is for the query_head
        self.score_threshold = test_cfg.get("score_thr", 0)
        if score_threshold is not None:
            self.score_threshold = score_threshold
        self.with_nms = False
        if "nms" in test_cfg:
            self.with_nms = True
            self.iou_threshold = test_cfg["nms"].get("iou_threshold", 0.8)
            if iou_threshold is not None:
                self.iou_threshold = iou_threshold
        nms = nms_settings(test_cfg, nms_type)
        if nms["forced_without_entry"]:   # a forced mode on a config without an nms entry: mmcv's default threshold
            self.with_nms = True
            self.iou_threshold = 0.3 if iou_threshold is None else iou_threshold
        self.nms_type, self.max_per_img = nms["type"], nms["max_per_img"]
        self.soft_method, self.min_score = nms["method"], nms["min_score"]
        self.soft = self.with_nms and self.nms_type == "soft_nms"
        pre = dict(self.cfg.model.data_preprocessor)
        if pre.pop("type") != "DetDataPreprocessor":
            raise AssertionError("data_preprocessor must be DetDataPreprocessor")
        self.mean = tuple(float(v) for v in pre.get("mean", (0.0, 0.0, 0.0)))
        self.std = tuple(float(v) for v in pre.get("std", (1.0, 1.0, 1.0)))
        self.pad_size_divisor = int(pre.get("pad_size_divisor", 1))
        self.pad_value = float(pre.get("pad_value", 0))   # DetDataPreprocessor: fills the divisor padding, AFTER normalisation
        # test pipeline: Resize(scale, keep_ratio) [+ Pad(size, pad_val)]
        self.scale, self.pad_size, self.pad_val = None, None, (0, 0, 0)
        for step in self.cfg.test_dataloader.dataset.pipeline:
            if step["type"] == "Resize":
                if not step.get("keep_ratio", False):
                    raise NotImplementedError("only keep_ratio=True resizing is on the reference's inference path")
                self.scale = tuple(step["scale"])
            elif step["type"] == "Pad":
                if step.get("size") is not None:
                    self.pad_size = tuple(step["size"])  # (width, height)
                pv = step.get("pad_val", dict(img=0))
                pv = pv.get("img", 0) if isinstance(pv, dict) else pv
                self.pad_val = tuple(pv) if isinstance(pv, (tuple, list)) else (pv,) * 3
        if self.scale is None:
            raise ValueError("Resize is not found in the test pipeline")
        self.tta = tta_settings(self.cfg, tta)
        self.ensemble = ensemble_settings(ensemble, self.tta)
        self.slicing = slicing_settings(slicing)
        if self.slicing is not None and self.tta is not None:
            raise NotImplementedError("slicing together with tta is not built: one or the other")
        self.visualizer = visualizer_settings(self.cfg, visualizer, dataset_meta)
        self._vis_tables = {}   # device -> (names, colors) on it: uploaded on the first visualising call there
        self.vis_format = vis_format_settings(vis_format)   # None: PNG files; a dict: JPEG files encoded on the GPU
        self.tracker = tracker_settings(tracker, self.cfg)
        self.track_association = track_association_setting(track_association, self.tracker)
        self._track_state = None   # [rows, state bytes] uint8 on the device of the first tracked call
        self._track_rows = {}      # stream -> its row of _track_state (and of _motion_state)
        self.track_motion = track_motion_settings(track_motion, self.tracker)
        self.track_motion_model = track_motion_model(track_motion)   # None, "translation" or "similarity"
        self._motion_state = None  # [rows, 16 + 160 * 160] uint8: every stream's last thumbnail, on the device
        self._chunk_streams = None   # the streams of the chunk __call__ is staging (a tracked call with track_motion)
        self._chunk_motion = None    # its [N, 4] motion on the device: _stage_call_chunk -> track_chunk
        self.track_appearance = track_appearance_settings(track_appearance, self.tracker)
        self._appearance_state = None   # [rows, max_tracks, 128] int16: every track's appearance, on the device
        self.redact = redact_settings(self.cfg, redact, dataset_meta, self.visualizer)
        self._redact_tables = {}   # device -> the class table on it: uploaded on the first redacting call there
        self.num_predicted_imgs = 0
        self.num_visualized_imgs = 0

    # ---- pre ------------------------------------------------------------------------------------------
    def preprocess(self, image: np.ndarray, device="cuda:0", dtype=torch.float32):
        """one RGB uint8 image [H, W, 3] -> (batch_inputs [1,3,Hp,Wp], img_masks [1,Hp,Wp], meta)"""
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("expected an RGB uint8 image of shape (H, W, 3)")
        H, W = image.shape[:2]
        nh, nw = rescale_size(H, W, self.scale)
        Hp, Wp = nh, nw
        if self.pad_size is not None:
            Wp, Hp = max(self.pad_size[0], nw), max(self.pad_size[1], nh)
        src = torch.from_numpy(np.ascontiguousarray(image)).to(device, non_blocking=True)
        # the pipeline's Pad: pad_val pixels, normalised with the image (mmdet Pad runs before DetDataPreprocessor)
        x, m = hip_ops.preprocess_image(src, (nh, nw), (Hp, Wp), self.mean, self.std, self.pad_val, dtype)
        d = self.pad_size_divisor
        if d > 1 and (Hp % d or Wp % d):
            # DetDataPreprocessor's own padding to a multiple of pad_size_divisor: applied to the NORMALISED tensor
            # and filled with pad_value (default 0), not with normalised pad_val pixels; the mask marks it as padding
            Hd, Wd = -(-Hp // d) * d, -(-Wp // d) * d
            x = torch.nn.functional.pad(x, (0, Wd - Wp, 0, Hd - Hp), value=self.pad_value)
            m = torch.nn.functional.pad(m, (0, Wd - Wp, 0, Hd - Hp), value=1.0)
            Hp, Wp = Hd, Wd
        meta = dict(ori_shape=(H, W), img_shape=(nh, nw), img_unpadded_shape=(nh, nw), pad_shape=(Hp, Wp),
                    scale_factor=(nw / W, nh / H))
        return x[None], m[None], meta

    def preprocess_batch(self, images: List[np.ndarray], device="cuda:0", dtype=torch.float32, input_format="rgb",
                         color=None):
        """RGB uint8 images [H_i, W_i, 3] -> (batch_inputs [N,3,H,W], img_masks [N,H,W], metas): per image the
        arithmetic of `preprocess`, stacked as mmdet's DetDataPreprocessor does (H, W = the largest Pad shape rounded
        up to pad_size_divisor; beyond an image's Pad region pad_value, mask 1).  One host-to-device copy, one launch
        per 32 images; dtype f16, bf16 or f32.  `input_format` / `color`: frames of another format or already on the
        GPU (`frame_settings`, `stage_chunk`)."""
        return self._preprocess_chunk(images, device, dtype, frame_settings(input_format, color))[:3]

    def _preprocess_chunk(self, images, device, dtype, frames=None):
        """preprocess_batch + the RGB buffer on the device and every image's (offset, H, W) in it, for the visualisation"""
        if not len(images):
            raise ValueError("preprocess_batch: no images")
        src, staged, _ = self._stage_call_chunk(images, device, frames)
        rows, metas = [], []
        d = self.pad_size_divisor
        for offset, H, W in staged:
            nh, nw = rescale_size(H, W, self.scale)
            Hp, Wp = nh, nw
            if self.pad_size is not None:
                Wp, Hp = max(self.pad_size[0], nw), max(self.pad_size[1], nh)
            rows.append((offset, H, W, nh, nw, Hp, Wp))
            pad_shape = (-(-Hp // d) * d, -(-Wp // d) * d) if d > 1 else (Hp, Wp)
            metas.append(dict(ori_shape=(H, W), img_shape=(nh, nw), img_unpadded_shape=(nh, nw), pad_shape=pad_shape,
                              scale_factor=(nw / W, nh / H)))
        Hb, Wb = max(m["pad_shape"][0] for m in metas), max(m["pad_shape"][1] for m in metas)
        for m in metas:
            m["batch_input_shape"] = (Hb, Wb)
        x, m = hip_ops.preprocess_batch(src, rows, (Hb, Wb), self.mean, self.std, self.pad_val, self.pad_value, dtype)
        return x, m, metas, src, staged

    # ---- post -----------------------------------------------------------------------------------------
    def postprocess_predictions(self, batch_boxes, batch_scores, batch_labels):
        """score threshold + per-class NMS per image (reference :380-400); with nms_type, the configured NMS and the
        max_per_img cut"""
        out = []
        for boxes, scores, labels in zip(batch_boxes, batch_scores, batch_labels):
            if self.score_threshold > 0:
                valid = scores > self.score_threshold
                scores, boxes, labels = scores[valid], boxes[valid], labels[valid]
            if self.soft:
                scores, keep = hip_ops.soft_nms(boxes, scores, labels, self.iou_threshold, self.soft_method,
                                                self.min_score)
                boxes, labels = boxes[keep], labels[keep]
            elif self.with_nms:
                keep = hip_ops.batched_nms(boxes, scores, labels, self.iou_threshold)
                boxes, scores, labels = boxes[keep], scores[keep], labels[keep]
            if self.max_per_img is not None:   # (after NMS the detections are in descending score order)
                boxes, scores, labels = boxes[:self.max_per_img], scores[:self.max_per_img], labels[:self.max_per_img]
            out.append((boxes, scores, labels))
        return out

    def run_inference(self, batch_inputs, img_masks, metas):
        """model + post-processing + rescale to the original image (reference :343-378)"""
        predictions = self.model(batch_inputs, img_masks)
        results = []
        for i, (boxes, scores, labels) in enumerate(self.postprocess_predictions(*predictions)):
            sf = metas[i]["scale_factor"]
            boxes = boxes / boxes.new_tensor([sf[0], sf[1], sf[0], sf[1]])
            results.append(dict(bboxes=boxes, scores=scores, labels=labels))
        return results

    @staticmethod
    def divisors(metas, dtype):
        """the rescale divisor [len(metas), 4] exactly as run_inference builds it (boxes.new_tensor of the Python floats)"""
        return torch.tensor([[m["scale_factor"][0], m["scale_factor"][1]] * 2 for m in metas], dtype=dtype)

    def postprocess_device(self, predictions, metas, div=None):
        """postprocess_batch's one launch, its result left on the device (hip_ops.Detections / SoftDetections); `div`:
        `divisors(metas, dtype)` already on the device"""
        boxes, scores, labels = predictions
        if div is None:
            div = self.divisors(metas, boxes.dtype).to(boxes.device)
        thr = self.score_threshold if self.score_threshold > 0 else None
        if self.soft:
            return hip_ops.postprocess_detections_soft(boxes, scores, labels, div, thr, self.iou_threshold,
                                                       self.soft_method, self.min_score, self.max_per_img)
        return hip_ops.postprocess_detections(boxes, scores, labels, div, thr,
                                              self.iou_threshold if self.with_nms else None)

    def postprocess_batch(self, predictions, metas):
        """the model's (boxes [N,Q,4], scores [N,Q], labels [N,Q]) -> one result dict per image ({"labels", "scores",
        "bboxes"} as Python lists, what `__call__` returns): score threshold, per-class NMS and / scale_factor of
        `run_inference` for the whole batch in one launch, then one device-to-host copy"""
        return self._postprocess_chunk(predictions, metas)[0]

    def _postprocess_chunk(self, predictions, metas):
        """postprocess_batch + the detections it fetched, still on the device"""
        dets = self.postprocess_device(predictions, metas)
        host = hip_ops.detections_to_host(dets)
        out = []
        for i in range(len(metas)):
            c = int(host.count[i])
            if self.max_per_img is not None:
                c = min(c, self.max_per_img)
            out.append({"labels": host.labels[i, :c].tolist(), "scores": host.scores[i, :c].float().tolist(),
                        "bboxes": host.boxes[i, :c].float().tolist()})
        return out, dets

    # ---- test-time augmentation ---------------------------------------------------------------------------
    def upload(self, images: List[np.ndarray], device="cuda:0", tail: Optional[torch.Tensor] = None):
        """RGB uint8 images back to back in one pinned staging buffer, one host-to-device copy -> (flat uint8 device
        buffer, the byte offset of every image, `tail` on the device).  `tail`: a small host tensor that rides in the
        same copy, 16-byte aligned behind the images (the TTA path's image widths and rescale divisors)."""
        offsets, offset = [], 0
        for image in images:
            if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
                raise ValueError("expected RGB uint8 images of shape (H, W, 3)")
            offsets.append(offset)
            offset += image.size
        if not offsets:
            raise ValueError("upload: no images")
        tail_at = -(-offset // 16) * 16
        tail_bytes = tail.contiguous().view(-1).view(torch.uint8) if tail is not None else None
        total = offset if tail is None else tail_at + tail_bytes.numel()
        staging = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        for image, o in zip(images, offsets):
            host[o:o + image.size] = np.ascontiguousarray(image).reshape(-1)
        if tail is not None:
            host[offset:tail_at] = 0
            staging[tail_at:] = tail_bytes
        dev = staging.to(device, non_blocking=True)
        return dev[:offset], offsets, (dev[tail_at:].view(tail.dtype).view(tail.shape) if tail is not None else None)

    @staticmethod
    def host_rgb(images, frames=None):
        """whether a chunk is what the reference's Inferencer takes: RGB frames, every one a host numpy array"""
        return (frames is None or frames["format"] == "rgb") and all(isinstance(im, np.ndarray) for im in images)

    def stage_chunk(self, images, device="cuda:0", frames=None, tail=None):
        """The chunk's frames as packed RGB HWC images in one flat uint8 buffer on the device
        -> (the buffer, [(offset, H, W)] per image, `tail` on the device).
        `frames`: `frame_settings(...)`, None for RGB.  `tail`: a small host tensor that rides in the chunk's one
        host-to-device copy, or a function of the [(offset, H, W)] list that returns one (the TTA and slicing tails
        depend on the frame sizes).
          * host RGB arrays: `upload` -- the images back to back in one pinned staging buffer, one copy, no launch;
          * any other host frame: its raw planes, rows packed, each plane 16-byte aligned, in the one pinned staging
            buffer (1.5 bytes per pixel of NV12 / I420 instead of 3) and one `hip_ops.frames_to_rgb` launch behind the
            copy;
          * JPEG files (`frames["format"] == "jpeg"`): only the headers are read on the host; the scans, as they are in
            the files, and their tables ride in the one pinned staging buffer and `hip_ops.jpeg_decode_staged` launches
            the decoder behind the copy.  The status words stay on the device until `check_jpeg_status`.  A file the
            GPU decoder does not support is decoded with Pillow and staged as an RGB frame of the same chunk;
          * GPU-resident frames: no upload; one launch per group of frames that share a storage, which read the planes
            where they lie (offsets relative to the storage, pitches from the strides).  With no host frame in the chunk
            the tail is a small copy of its own.
        Host and GPU frames may be mixed.  The images of a converted chunk start at multiples of 16 bytes."""
        if not len(images):
            raise ValueError("stage_chunk: no images")
        if frames is not None and frames["format"] == "jpeg":
            return self._stage_jpeg_chunk(images, device, frames, tail)
        if self.host_rgb(images, frames):
            shapes = []
            for image in images:
                if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
                    raise ValueError("expected RGB uint8 images of shape (H, W, 3)")
                shapes.append(image.shape[:2])
            offsets = np.cumsum([0] + [H * W * 3 for H, W in shapes]).tolist()
            staged = [(o, H, W) for o, (H, W) in zip(offsets, shapes)]
            src, _, tail = self.upload(images, device, tail(staged) if callable(tail) else tail)
            return src, staged, tail
        frames = frames or frame_settings()
        items = [parse_frame(im, frames["format"]) for im in images]
        staged, dst_bytes = [], 0
        for it in items:
            staged.append((dst_bytes, it.H, it.W))
            dst_bytes = -(-(dst_bytes + it.H * it.W * 3) // 16) * 16
        if callable(tail):
            tail = tail(staged)
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        host_rows, copies, groups, pos = [], [], {}, 0   # groups: storage address -> (its bytes as a flat tensor, rows)
        for it, (dst, H, W) in zip(items, staged):
            cols = []
            for plane in it.planes:
                if it.resident:
                    cols += [plane.storage_offset(), plane.stride(0)]
                else:
                    pos = -(-pos // 16) * 16
                    copies.append((pos, plane))
                    cols += [pos, plane.shape[1]]
                    pos += plane.size
            row = (it.code, H, W) + tuple(cols) + (0,) * (6 - len(cols)) + (dst,)
            if not it.resident:
                host_rows.append(row)
                continue
            if it.planes[0].device != dev:
                raise ValueError(f"a GPU-resident frame on {it.planes[0].device} in a call for {dev}")
            storage = it.planes[0].untyped_storage()
            if storage.data_ptr() not in groups:
                flat = torch.empty((0,), dtype=torch.uint8, device=dev).set_(storage, 0, (storage.nbytes(),), (1,))
                groups[storage.data_ptr()] = (flat, [])
            groups[storage.data_ptr()][1].append(row)
        tail_at = -(-pos // 16) * 16
        tail_bytes = tail.contiguous().view(-1).view(torch.uint8) if tail is not None else None
        total = pos if tail is None else tail_at + tail_bytes.numel()
        up = None
        if total:
            staging = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
            host = staging.numpy()
            for at, plane in copies:
                host[at:at + plane.size].reshape(plane.shape)[...] = plane
            if tail is not None:
                staging[tail_at:] = tail_bytes
            up = staging.to(dev, non_blocking=True)
        src = torch.empty((dst_bytes,), dtype=torch.uint8, device=dev)
        if host_rows:
            hip_ops.frames_to_rgb(up[:pos], host_rows, dst_bytes, frames["matrix"], frames["range"], out=src)
        for flat, rows in groups.values():
            hip_ops.frames_to_rgb(flat, rows, dst_bytes, frames["matrix"], frames["range"], out=src)
        return src, staged, (up[tail_at:].view(tail.dtype).view(tail.shape) if tail is not None else None)

    def _stage_jpeg_chunk(self, images, device, frames, tail):
        """stage_chunk for JPEG files"""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        first = getattr(self, "_chunk_start", 0)
        parsed, items, names = [], [], []
        for i, item in enumerate(images):
            data = hip_ops.jpeg_file_bytes(item)
            rc, info, tables = hip_ops.jpeg_parse(data)
            if rc == 0:
                items.append(len(parsed))
                parsed.append((data, info, tables))
                names.append(f"image {first + i}")
                continue
            reason = hip_ops.jpeg_reason(rc, info)
            if reason in ("bad_header", "too_large"):
                raise ValueError(f"input_format='jpeg': image {first + i}: {reason}")
            rgb = hip_ops.jpeg_host_decode(data)
            if rgb is None:
                raise ValueError(f"input_format='jpeg': image {first + i}: {reason} files are not decoded on the GPU and "
                                 "Pillow is not installed for the host fallback")
            items.append(parse_frame(rgb, "rgb"))
        staged, dst_bytes = [], 0
        for it in items:
            H, W = (int(parsed[it][1][0]), int(parsed[it][1][1])) if isinstance(it, int) else (it.H, it.W)
            staged.append((dst_bytes, H, W))
            dst_bytes = -(-(dst_bytes + H * W * 3) // 16) * 16
        if callable(tail):
            tail = tail(staged)
        host_rows, copies, pos = [], [], 0
        for it, (dst, H, W) in zip(items, staged):
            if not isinstance(it, int):
                pos = -(-pos // 16) * 16
                copies.append((pos, it.planes[0]))
                host_rows.append((it.code, H, W, pos, it.planes[0].shape[1], 0, 0, 0, 0, dst))
                pos += it.planes[0].size
        planes_end = pos
        scan_copies, groups, scan_at, pos = hip_ops.jpeg_stage(parsed, pos)
        tail_at = -(-pos // 16) * 16
        tail_bytes = tail.contiguous().view(-1).view(torch.uint8) if tail is not None else None
        total = pos if tail is None else tail_at + tail_bytes.numel()
        staging = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        for at, plane in copies:
            host[at:at + plane.size].reshape(plane.shape)[...] = plane
        for at, part in scan_copies:
            host[at:at + part.size] = part
        if tail is not None:
            staging[tail_at:] = tail_bytes
        up = staging.to(dev, non_blocking=True)
        src = torch.empty((dst_bytes,), dtype=torch.uint8, device=dev)
        if host_rows:
            hip_ops.frames_to_rgb(up[:planes_end], host_rows, dst_bytes, frames["matrix"], frames["range"], out=src)
        if parsed:
            dst_offsets = [staged[i][0] for i, it in enumerate(items) if isinstance(it, int)]
            status = hip_ops.jpeg_decode_staged(up, parsed, groups, scan_at, dst_offsets, src)
            self._jpeg_pending = getattr(self, "_jpeg_pending", []) + [(status, names)]
        return src, staged, (up[tail_at:].view(tail.dtype).view(tail.shape) if tail is not None else None)

    def check_jpeg_status(self):
        """Fetches the status words of the JPEG chunks staged since the last call and raises ValueError for the first
        file whose scan did not decode.  `__call__` does this behind each chunk's download of its detections, so the
        decoder adds no synchronisation in front of the forward."""
        pending, self._jpeg_pending = getattr(self, "_jpeg_pending", []), []
        for status, names in pending:
            err = hip_ops.jpeg_status_error(status.cpu().numpy(), names)
            if err is not None:
                raise err

    def view_rows(self, offsets, shapes, scale, flips):
        """One TTA scale of a chunk: images of `shapes` (H, W) at byte `offsets`, resized keep-ratio into `scale`, once
        per entry of `flips` (False / True: mirrored), padded to pad_size_divisor and stacked.  Rows are flip-major --
        row f * N + n is image n under flips[f] -- so the post-processed result reshapes to [len(flips), N, Q].
        -> (rows for hip_ops.preprocess_views, metas per row, (H, W) of the batch)"""
        d = self.pad_size_divisor
        rows, metas = [], []
        for f in flips:
            for o, (H, W) in zip(offsets, shapes):
                nh, nw = rescale_size(H, W, scale)
                rows.append((o, H, W, nh, nw, nh, nw, 1 if f else 0))
                pad_shape = (-(-nh // d) * d, -(-nw // d) * d) if d > 1 else (nh, nw)
                metas.append(dict(ori_shape=(H, W), img_shape=(nh, nw), img_unpadded_shape=(nh, nw), pad_shape=pad_shape,
                                  scale_factor=(nw / W, nh / H), flip=bool(f)))
        Hb, Wb = max(m["pad_shape"][0] for m in metas), max(m["pad_shape"][1] for m in metas)
        for m in metas:
            m["batch_input_shape"] = (Hb, Wb)
        return rows, metas, (Hb, Wb)

    def tta_batch(self, images: List[np.ndarray], device="cuda:0", dtype=torch.float32, input_format="rgb", color=None):
        """one chunk through every view and the merge -> one result dict per image (see the module docstring).  The
        chunk's one upload carries the images, their widths (fp32, for the un-flip) and every view's rescale divisor."""
        return self._tta_chunk(images, device, dtype, frame_settings(input_format, color))[0]

    def _tta_chunk(self, images, device, dtype, frames=None):
        """tta_batch + the RGB buffer on the device, every image's (offset, H, W) and the merged detections on the device"""
        t = self.tta
        flips = (False, True) if t["flip"] else (False,)
        N, plans = len(images), []

        def tail_of(staged):
            shapes = [(H, W) for _, H, W in staged]
            plans.extend(self.view_rows([o for o, _, _ in staged], shapes, scale, flips) for scale in t["scales"])
            widths = torch.tensor([float(w) for _, w in shapes], dtype=torch.float32)
            div = torch.cat([self.divisors(metas, dtype) for _, metas, _ in plans])      # [S * F * N, 4]
            return torch.cat((widths.view(torch.uint8), div.view(-1).view(torch.uint8)))

        src, staged, tail = self._stage_call_chunk(images, device, frames, tail_of)
        widths = tail[:4 * N].view(torch.float32)
        div = tail[4 * N:].view(dtype).view(len(plans), len(flips) * N, 4)
        view_dets = [[] for _ in range(1 + len(self.ensemble))]   # per model, its scales in order
        total = len(t["views"]) * (1 + len(self.ensemble))
        for s, (rows, metas, batch_hw) in enumerate(plans):
            x, m = hip_ops.preprocess_views(src, rows, batch_hw, self.mean, self.std, self.pad_val, self.pad_value, dtype)
            preds = self.model(x, m)
            Q = preds[1].shape[1]
            if s == 0 and total * Q > hip_ops.TTA_MAX_CANDIDATES:   # (Q is the model's: known after a forward)
                raise ValueError(f"tta: {total} views of {Q} detections exceed the merge kernel's "
                                 f"{hip_ops.TTA_MAX_CANDIDATES} candidates per image")
            view_dets[0].append(self.postprocess_device(preds, metas, div[s]))
            for k, model in enumerate(self.ensemble, 1):   # the further models on the same pre-processed views
                preds_k = model(x, m)
                if preds_k[1].shape[1] != Q:
                    raise ValueError(f"ensemble: model {k} returns {preds_k[1].shape[1]} detections per image, the main "
                                     f"model {Q}: the merged views need one Q")
                view_dets[k].append(self.postprocess_device(preds_k, metas, div[s]))
        view_dets = [d for per_model in view_dets for d in per_model]   # v = (k * S + s) * F + f
        view_flips = [f for _, f in t["views"]] * (1 + len(self.ensemble))
        if t["wbf"] is not None:
            dets = hip_ops.wbf_merge(view_dets, view_flips, widths, t["wbf"], t["max_per_img"])
        else:
            dets = hip_ops.tta_merge(view_dets, view_flips, widths, t["nms"], t["max_per_img"])
        host = hip_ops.detections_to_host(dets)
        out = []
        for i in range(N):
            c = int(host.count[i])
            out.append({"labels": host.labels[i, :c].tolist(), "scores": host.scores[i, :c].float().tolist(),
                        "bboxes": host.boxes[i, :c].float().tolist()})
            if t["wbf"] is not None:
                out[-1]["votes"] = host.votes[i, :c].tolist()
        return out, src, staged, dets

    # ---- sliced inference -------------------------------------------------------------------------------------
    @staticmethod
    def slice_grid(H, W, tile, overlap):
        """the tiles of an H x W image: `tile` (w, h), `overlap` a ratio or (ox, oy), each in [0, 1).  Per axis of length
        L with tile t and overlap o the step is t - int(o * t) (at least 1); tiles start at 0, step, 2 step, ... up to
        and including the first that reaches L, which is moved back to end at L (an axis shorter than t: one tile of
        length L).  -> [(y0, x0, h, w)], y-major, then x"""
        ox, oy = tuple(overlap) if isinstance(overlap, (tuple, list)) else (overlap, overlap)

        def axis(L, t, o):
            if not 0 <= o < 1 or t < 1 or L < 1:
                raise ValueError("slice_grid: positive sizes and an overlap in [0, 1)")
            step, starts, p = max(1, t - int(o * t)), [], 0
            while p + t < L:
                starts.append(p)
                p += step
            return starts + [max(0, L - t)], min(t, L)

        (xs, w), (ys, h) = axis(int(W), int(tile[0]), ox), axis(int(H), int(tile[1]), oy)
        return [(y, x, h, w) for y in ys for x in xs]

    @staticmethod
    def slice_limits(views, Q=None):
        """the merge kernel's limits: `views` of one image (tiles + the whole image), Q detections per view once known"""
        if views > hip_ops.SLICE_MAX_VIEWS:
            raise ValueError(f"slicing: {views} views of an image, at most {hip_ops.SLICE_MAX_VIEWS} (tiles + the whole "
                             "image) are merged: use larger tiles")
        if Q is not None and views * Q > hip_ops.TTA_MAX_CANDIDATES:
            raise ValueError(f"slicing: {views} views of {Q} detections exceed the merge kernel's "
                             f"{hip_ops.TTA_MAX_CANDIDATES} candidates per image")

    def slice_rows(self, offsets, shapes):
        """The rows of a chunk: every image of `shapes` (H, W) at byte `offsets` as its tiles (and, with full_image, the
        whole image last), each resized keep-ratio into the config's scale as `view_rows` treats an image, padded to
        pad_size_divisor and stacked; image-major.  -> (rows for hip_ops.preprocess_tiles, metas per row with `origin`
        (x0, y0), the [N, V] view table (-1: no such view), (H, W) of the batch)"""
        s, d = self.slicing, self.pad_size_divisor
        rows, metas, table = [], [], []
        for o, (H, W) in zip(offsets, shapes):
            views = self.slice_grid(H, W, s["tile"], s["overlap"]) + ([(0, 0, H, W)] if s["full_image"] else [])
            self.slice_limits(len(views))
            table.append(list(range(len(rows), len(rows) + len(views))))
            for y0, x0, h, w in views:
                nh, nw = rescale_size(h, w, self.scale)
                rows.append((o, H, W, y0, x0, h, w, nh, nw, nh, nw))
                pad_shape = (-(-nh // d) * d, -(-nw // d) * d) if d > 1 else (nh, nw)
                metas.append(dict(ori_shape=(h, w), img_shape=(nh, nw), img_unpadded_shape=(nh, nw), pad_shape=pad_shape,
                                  scale_factor=(nw / w, nh / h), origin=(x0, y0)))
        Hb, Wb = max(m["pad_shape"][0] for m in metas), max(m["pad_shape"][1] for m in metas)
        for m in metas:
            m["batch_input_shape"] = (Hb, Wb)
        V = max(len(t) for t in table)
        return rows, metas, [t + [-1] * (V - len(t)) for t in table], (Hb, Wb)

    def slice_batch(self, images: List[np.ndarray], device="cuda:0", dtype=torch.float32, input_format="rgb",
                    color=None):
        """one chunk through every tile and the merge -> one result dict per image (see the module docstring).  The
        chunk's one upload carries the images, every row's origin and rescale divisor, the image sizes and the view table."""
        return self._slice_chunk(images, device, dtype, frame_settings(input_format, color))[0]

    def _slice_chunk(self, images, device, dtype, frames=None):
        """slice_batch + the RGB buffer on the device, every image's (offset, H, W) and the merged detections on the device"""
        s = self.slicing
        N, plan = len(images), []

        def tail_of(staged):
            shapes = [(H, W) for _, H, W in staged]
            plan.extend(self.slice_rows([o for o, _, _ in staged], shapes))
            metas, table = plan[1], plan[2]
            origins = torch.tensor([m["origin"] for m in metas], dtype=torch.float32)            # [R, 2] (x0, y0)
            sizes = torch.tensor([[float(W), float(H)] for H, W in shapes], dtype=torch.float32)  # [N, 2] (W, H)
            view_rows = torch.tensor(table, dtype=torch.int32)                                    # [N, V]
            div = self.divisors(metas, dtype)                                                     # [R, 4]
            return torch.cat([t.view(-1).view(torch.uint8) for t in (origins, sizes, view_rows, div)])

        src, staged, tail = self._stage_call_chunk(images, device, frames, tail_of)
        rows, metas, table, batch_hw = plan
        R, V = len(rows), len(table[0])
        origins = tail[:8 * R].view(torch.float32).view(R, 2)
        sizes = tail[8 * R:8 * (R + N)].view(torch.float32).view(N, 2)
        view_rows = tail[8 * (R + N):8 * (R + N) + 4 * N * V].view(torch.int32).view(N, V)
        div = tail[8 * (R + N) + 4 * N * V:].view(dtype).view(R, 4)
        x, m = hip_ops.preprocess_tiles(src, rows, batch_hw, self.mean, self.std, self.pad_val, self.pad_value, dtype)
        row_dets = []
        for i in range(0, R, s["tile_batch"]):
            j = min(R, i + s["tile_batch"])
            preds = self.model(x[i:j], m[i:j])
            if i == 0:   # (Q is the model's: known after a forward)
                self.slice_limits(V, preds[1].shape[1])
            row_dets.append(self.postprocess_device(preds, metas[i:j], div[i:j]))
        dets = hip_ops.slice_merge(row_dets, view_rows, origins, sizes, s["merge"], s["max_per_img"])
        host = hip_ops.detections_to_host(dets)
        out = []
        for i in range(N):
            c = int(host.count[i])
            out.append({"labels": host.labels[i, :c].tolist(), "scores": host.scores[i, :c].float().tolist(),
                        "bboxes": host.boxes[i, :c].float().tolist()})
        return out, src, staged, dets

    # ---- tracking ---------------------------------------------------------------------------------------------
    def reset_tracks(self, stream=None):
        """forget the tracks of one stream, or of all (None): its state is zeroed, ids start at 1 again; with
        track_motion its last thumbnail goes too (the stream's next frame has no motion), with track_appearance the
        appearances of its tracks"""
        if stream is None:
            self._track_state, self._track_rows, self._motion_state, self._appearance_state = None, {}, None, None
        elif hip_ops.track_streams(stream, 1)[0] in self._track_rows:
            for state in (self._track_state, self._motion_state, self._appearance_state):
                if state is not None and self._track_rows[int(stream)] < state.shape[0]:
                    state[self._track_rows[int(stream)]].zero_()

    def _stream_state(self, state, new, streams, dev):
        """the state tensor of `streams` (`new(rows)` makes a fresh one), grown to hold the row of every stream seen"""
        if state is not None and state.device != dev:
            raise ValueError(f"the track states live on {state.device}: reset_tracks() before a call on {dev}")
        for s in streams:
            self._track_rows.setdefault(s, len(self._track_rows))
        have = 0 if state is None else state.shape[0]
        if len(self._track_rows) > have:   # (grows by doubling: a new camera is rare)
            grown = new(max(len(self._track_rows), 2 * have))
            if have:
                grown[:have].copy_(state)
            state = grown
        return state

    def _stage_call_chunk(self, images, device, frames, tail=None):
        """stage_chunk for a chunk of __call__: with track_motion the camera-motion estimate of the chunk's own images
        (whole frames, not views or tiles) is launched behind the staging -- in front of the forward, and of draw_chunk,
        which draws into that buffer.  The motion stays on the device for track_chunk."""
        src, staged, tail = self.stage_chunk(images, device, frames, tail)
        self._chunk_motion = None
        if self.track_motion is not None and self._chunk_streams is not None:
            self._motion_state = self._stream_state(self._motion_state, lambda n: hip_ops.new_motion_state(n, src.device),
                                                    self._chunk_streams, src.device)
            self._chunk_motion, _ = hip_ops.estimate_motion(src, staged, self._motion_state,
                                                            [self._track_rows[s] for s in self._chunk_streams],
                                                            self.track_motion, model=self.track_motion_model)
        return src, staged, tail

    def track_chunk(self, dets, streams, src=None, src_rows=None):
        """the track ids of a chunk's final detections: one hip_ops.track_update launch on the states kept on the device
        and one device-to-host copy -> [N, Q] int32 numpy.  A stream's state is created on its first frame.  With
        track_motion the chunk's motion (_stage_call_chunk) feeds the launch and its copy follows the ids':
        -> (ids, [N, 4] float32 numpy, or [N, 8] under "similarity").  With track_appearance one
        hip_ops.appearance_descriptors launch on the chunk's RGB buffer `src` (images `src_rows`: still undrawn) goes in
        front, and the tracking launch takes the descriptors and the streams' appearance states."""
        dev = dets.scores.device
        T = self.tracker["max_tracks"]
        self._track_state = self._stream_state(self._track_state, lambda n: hip_ops.new_track_state(n, T, dev), streams, dev)
        rows = [self._track_rows[s] for s in streams]
        app = {}
        if self.track_appearance is not None:
            self._appearance_state = self._stream_state(self._appearance_state,
                                                        lambda n: hip_ops.new_appearance_state(n, T, dev), streams, dev)
            if self._appearance_state.shape[0] != self._track_state.shape[0]:   # (the two grow together)
                raise RuntimeError("the appearance states and the track states hold different numbers of streams")
            app = dict(appearance=hip_ops.appearance_descriptors(src, src_rows, dets),
                       appearance_state=self._appearance_state, appearance_settings=self.track_appearance)
        if self.track_motion is None:
            return hip_ops.track_update(dets, self._track_state, rows, self.tracker, self.track_association,
                                        **app).cpu().numpy()
        ids = hip_ops.track_update(dets, self._track_state, rows, self.tracker, self.track_association,
                                   motion=self._chunk_motion, **app)
        return ids.cpu().numpy(), self._chunk_motion.cpu().numpy()

    # ---- visualisation and files --------------------------------------------------------------------------
    def download_chunk(self, src, rows):
        """one device-to-host copy of the chunk's RGB buffer -> one [H, W, 3] uint8 array per image"""
        VIS_DOWNLOADS["rgb"] += 1
        host = src.cpu().numpy()
        return [host[o:o + H * W * 3].reshape(H, W, 3).copy() for o, H, W in rows]

    def draw_chunk(self, src, rows, dets, pred_score_thr, download=True):
        """the chunk's predictions drawn on its uploaded images: one hip_ops.draw_detections launch on the buffer the
        preprocessing read (in place, after it on the same stream) and one device-to-host copy of that buffer -> one
        [H, W, 3] uint8 array per image (download=False: no copy, None per image -- the drawn images stay in `src`)"""
        v = self.visualizer
        key = str(src.device)
        if key not in self._vis_tables:
            self._vis_tables[key] = (v["names"].to(src.device), v["colors"].to(src.device))
        names, colors = self._vis_tables[key]
        hip_ops.draw_detections(src, rows, self._clamped(dets), names, colors,
                                dict(v["style"], score_thr=float(pred_score_thr)))
        return self.download_chunk(src, rows) if download else [None] * len(rows)

    def _clamped(self, dets):
        """the chunk's final detections as the predictions keep them: the hard path cuts to max_per_img on the host
        (postprocess_batch), so a kernel that follows the predictions gets the clamped count"""
        if self.max_per_img is not None and not self.soft and self.tta is None and self.slicing is None:
            return dets._replace(count=dets.count.clamp(max=self.max_per_img))
        return dets

    def redact_chunk(self, src, rows, dets):
        """the chunk's detected regions redacted in its uploaded images: hip_ops.redact_detections on the buffer the
        preprocessing read, in place and on the same stream -- behind track_chunk (the appearance descriptors read the
        original pixels), in front of draw_chunk and encode_jpeg.  No copy, no synchronisation."""
        select = self.redact["select"]
        if select is not None:
            key = str(src.device)
            if key not in self._redact_tables:
                self._redact_tables[key] = select.to(src.device)
            select = self._redact_tables[key]
        hip_ops.redact_detections(src, rows, self._clamped(dets), self.redact["style"], select)

    def save_outputs(self, pred, vis, out_dir, no_save_pred, jpeg=None):
        """the files of one image (reference pred2dict :303-341, visualize :214-219): vis/%08d.png from the array `vis`,
        or, with a JPEG vis_format, the reference's vis/%08d.jpg from the encoded file `jpeg`"""
        if out_dir == "":
            return
        if not no_save_pred:
            os.makedirs(os.path.join(out_dir, "preds"), exist_ok=True)
            with open(os.path.join(out_dir, "preds", f"{self.num_predicted_imgs}.json"), "w") as f:
                json.dump(pred, f)
        if jpeg is not None:
            os.makedirs(os.path.join(out_dir, "vis"), exist_ok=True)
            with open(os.path.join(out_dir, "vis", "%08d.jpg" % self.num_visualized_imgs), "wb") as f:
                f.write(jpeg)
        elif vis is not None:
            os.makedirs(os.path.join(out_dir, "vis"), exist_ok=True)
            write_png(os.path.join(out_dir, "vis", "%08d.png" % self.num_visualized_imgs), vis)

    def __call__(self, images: List[np.ndarray], return_vis: bool = False, show: bool = False, wait_time: int = 0,
                 no_save_vis: bool = False, draw_pred: bool = True, pred_score_thr: float = 0.3,
                 return_datasamples: bool = False, print_result: bool = False, no_save_pred: bool = True,
                 out_dir: str = "", device: str = "cuda:0", dtype: torch.dtype = torch.float32,
                 batch_size: int = 1, input_format: str = "rgb", color=None, streams=None) -> Dict:
        if show or return_datasamples or (return_vis and self.visualizer is None and self.redact is None):
            raise NotImplementedError("visualisation / DetDataSample / file output need mmengine + cv2: not part of this build")
        if int(batch_size) != batch_size or batch_size < 1:
            raise ValueError(f"batch_size must be a positive integer, got {batch_size}")
        batch_size = int(batch_size)
        frames = frame_settings(input_format, color)
        plain = self.host_rgb(images, frames)   # what the reference takes; everything else is staged per chunk
        results_dict = {"predictions": [], "visualization": []}
        save_vis = out_dir != "" and not no_save_vis
        # (with `redact` the images come out without a visualiser too: redacted and undrawn)
        visualise = (self.visualizer is not None or self.redact is not None) and bool(return_vis or save_vis)
        if isinstance(return_vis, str):
            if return_vis != "jpeg" or self.vis_format is None:
                raise ValueError('return_vis="jpeg" needs Inferencer(..., vis_format="jpeg"); otherwise pass a bool')
            results_dict["visualization_jpeg"] = []
        # a JPEG vis_format: the files come from the encoder, the arrays only when the caller asked for them
        want_jpeg = visualise and self.vis_format is not None and (save_vis or return_vis == "jpeg")
        want_arrays = visualise and (self.vis_format is None or (bool(return_vis) and return_vis != "jpeg"))
        if self.tracker is not None:
            streams = hip_ops.track_streams(streams, len(images))
        elif streams is not None:
            raise ValueError("streams without a tracker: Inferencer(..., tracker=dict(...)) turns tracking on")
        if (batch_size == 1 and dtype != torch.bfloat16 and not self.soft and self.tta is None and self.slicing is None
                and not visualise and plain and self.tracker is None):
            for image in images:
                with torch.no_grad():
                    x, m, meta = self.preprocess(image, device, dtype)
                    res = self.run_inference(x, m, [meta])[0]
                pred = {"labels": res["labels"].tolist(), "scores": res["scores"].float().tolist(),
                        "bboxes": res["bboxes"].float().tolist()}
                if self.redact is not None:   # (no image leaves this call: the rows it would redact, nothing launched)
                    pred["redacted"] = redacted_rows(pred, self.redact)
                if print_result:
                    print(pred)
                self.save_outputs(pred, None, out_dir, no_save_pred)
                self.num_predicted_imgs += 1
                results_dict["predictions"].append(pred)
            return results_dict
        for start in range(0, len(images), batch_size):
            chunk = images[start:start + batch_size]
            self._chunk_start = start
            self._chunk_streams = streams[start:start + batch_size] if self.track_motion is not None else None
            with torch.no_grad():
                if self.tta is not None:
                    preds, src, rows, dets = self._tta_chunk(chunk, device, dtype, frames)
                elif self.slicing is not None:
                    preds, src, rows, dets = self._slice_chunk(chunk, device, dtype, frames)
                else:
                    x, m, metas, src, rows = self._preprocess_chunk(chunk, device, dtype, frames)
                    preds, dets = self._postprocess_chunk(self.model(x, m), metas)
                if frames["format"] == "jpeg":   # (the detections are on the host: the status words cost no wait)
                    self.check_jpeg_status()
                if self.tracker is not None:   # the ids of the rows the predictions kept (a host-side cut included)
                    ids = self.track_chunk(dets, streams[start:start + batch_size], src, rows)
                    if self.track_motion is not None:
                        ids, motion = ids
                        for pred, m in zip(preds, motion):
                            pred["camera_motion"] = [float(m[0]), float(m[1])] if m[2] == 1.0 else None
                            if self.track_motion_model == "similarity":
                                pred["camera_transform"] = camera_transform(m)
                    for pred, row in zip(preds, ids):
                        pred["track_ids"] = row[:len(pred["labels"])].tolist()
                    self._chunk_streams = None
                drawn = [None] * len(chunk)
                if self.redact is not None:
                    for pred in preds:
                        pred["redacted"] = redacted_rows(pred, self.redact)
                    if visualise:   # behind the descriptors, in front of the drawing and the encoder
                        self.redact_chunk(src, rows, dets)
                if visualise and draw_pred and self.visualizer is not None:
                    drawn = self.draw_chunk(src, rows, dets, pred_score_thr, download=want_arrays)
                elif want_arrays and plain and self.redact is None:
                    # the originals, as mmdet returns the undrawn image; nothing launched
                    drawn = [im.copy() for im in chunk]
                elif want_arrays:             # the undrawn converted frames: one download of the chunk's RGB buffer
                    drawn = self.download_chunk(src, rows)
                files = [None] * len(chunk)
                if want_jpeg:   # on the images where the kernels left them: only the compressed bytes come back
                    files = hip_ops.encode_jpeg(src, rows, self.vis_format["quality"], self.vis_format["subsampling"])
            for pred, vis, jpeg in zip(preds, drawn, files):
                if print_result:
                    print(pred)
                self.save_outputs(pred, vis if save_vis else None, out_dir, no_save_pred, jpeg if save_vis else None)
                self.num_predicted_imgs += 1
                if vis is not None or jpeg is not None:
                    self.num_visualized_imgs += 1
                    if vis is not None and return_vis and return_vis != "jpeg":
                        results_dict["visualization"].append(vis)
                    if return_vis == "jpeg":
                        results_dict["visualization_jpeg"].append(jpeg)
                results_dict["predictions"].append(pred)
        return results_dict
