/* codetr_wbf.h -- companion header of codetr_hip.h: weighted boxes fusion (WBF) of the detections of several views of an
 * image -- test-time augmentation's scales and flips, or the same views run through several models -- on the GPU, one
 * workgroup per image.  Exported from the same libcodetr_hip.so; versioned on its own (a self-contained addition does not
 * touch CODETR_HIP_ABI_VERSION).  Error codes and CODETR_TTA_MAX_VIEWS are codetr_hip.h's.
 *
 * Beyond the reference (its Inferencer runs one view through one model).  The algorithm is Solovyev, Wang and Gabruseva,
 * "Weighted boxes fusion: ensembling boxes from different object detection models" (2021), as their `ensemble_boxes`
 * package runs it with conf_type 'avg' or 'max' and allows_overflow=False: where codetr_tta_merge_* keeps one view's box of
 * every group and discards the others, WBF clusters the views' boxes per class and emits the confidence-weighted mean box
 * of every cluster, with a score that says how many views agreed.  `ensemble_boxes` is not installed where this is tested:
 * PARITY IS UNPINNED.  The rule below is this library's, stated operation by operation so that a restatement
 * (tests/wbf_ref.py) reproduces every bit.  Two deviations from the package are deliberate:
 *   the tie rule   a candidate that overlaps two clusters equally joins the one whose founder has the lowest candidate
 *                  index; the package takes the cluster created first (its founder has the higher confidence);
 *   live           a candidate takes part iff score >= skip_box_thr and score * weight > 0; the package drops
 *                  score < skip_box_thr and keeps zero-confidence boxes (which can only divide by zero).
 * The two model-aware confidence types and allows_overflow=True are not built.
 *
 * codetr_wbf_merge_*: the operands are those of codetr_tta_merge_* (codetr_hip.h, "Test-time augmentation"):
 *     boxes_dev [V, N, Q, 4], scores_dev [V, N, Q] in T; labels_dev [V, N, Q] int64; count_dev [V, N] int32: rows
 *     j < count[v, n] of view v are image n's candidates; flip_mask: bit v set = view v was flipped; width_dev [N] fp32:
 *     the original image width W.  The candidate index is c = v * Q + j.
 *     weights_host   HOST [V] fp32, the weight of every view (NULL: all 1); conf_type CODETR_WBF_CONF_AVG / _MAX;
 *     iou_threshold, skip_box_thr, max_keep as below.
 *   Everything is fp32 with one rounding per operation, never contracted into an FMA:
 *     1. boxes and scores convert to fp32 (exact); a flipped view's box becomes (W - x2, y1, W - x1, y2), one rounding per
 *        coordinate (step 1 of codetr_tta_merge_*).  conf_c = score_c * weight[v], one rounded product.  wsum = the sum
 *        of the weights in view order, V rounded additions starting from 0; wmax = their maximum.  Candidate c is live
 *        iff score_c >= skip_box_thr and conf_c > 0 (a NaN fails both).
 *     2. per label, the live candidates are processed by conf descending (codetr_postprocess_detections_*'s order), ties
 *        to the lowest c.
 *     3. for candidate c and every cluster k of its label: the fused box F_k = (SX1_k / SC_k, SY1_k / SC_k, SX2_k / SC_k,
 *        SY2_k / SC_k), four IEEE divisions; ovr = inter / (area_F + area_c - inter), the arithmetic of
 *        codetr_postprocess_softnms_* between F_k and box c, with area_F = (F.x2 - F.x1) * (F.y2 - F.y1) one rounded
 *        product of the fused coordinates.  c joins the cluster with the highest ovr among those with
 *        ovr > iou_threshold (a NaN compares false; -0 equals +0); ties go to the cluster whose founder has the lowest c.
 *     4. no cluster matched: c founds one with SX1 = conf_c * x1 (one rounded product; SY1, SX2, SY2 likewise),
 *        SC = conf_c, n = 1, top = conf_c.  Otherwise SX1 += conf_c * x1 (the product rounded, then the sum rounded; the
 *        others likewise), SC += conf_c, n += 1.
 *     5. every cluster emits: the box F_k; the label; index = its founder's c; votes = n; the score
 *          CODETR_WBF_CONF_AVG   ((SC / (float)n) * fminf((float)n, wsum)) / wsum
 *          CODETR_WBF_CONF_MAX   top / wmax
 *     6. the rows are sorted by score descending (the order of step 2), ties by ascending founder c; the first max_keep
 *        stay (max_keep <= 0: all).
 *   Outputs, K = max_keep (V * Q when max_keep <= 0): boxes_out_dev [N, K, 4], scores_out_dev [N, K] in T (the fp32
 *   value rounded once), labels_out_dev [N, K] int64, index_out_dev [N, K] int32, count_out_dev [N] int32,
 *   votes_out_dev [N, K] int32; rows beyond count_out[n] are zero.
 *   The kernel (csrc/prepost.hip, wbf_merge_kernel) has codetr_tta_merge_*'s front end -- one workgroup of 1024 threads
 *   per image, the candidates sorted by (label, c) -- then one wave per label segment walks steps 2 to 5 with no workgroup
 *   barrier: a wave maximum picks the next candidate, every lane measures it against the clusters it owns, a second wave
 *   maximum names the winner, whose lane updates the sums in the founder's slots.  All candidates stay in LDS (36 bytes
 *   per slot of the power of two >= V * Q, 144 KB at 4096): no workspace operand.
 *   CODETR_E_BADARG for a null pointer (weights_host may be NULL), V, N or Q <= 0, a flip bit at or above V, a conf_type
 *   other than the two below, an iou_threshold or skip_box_thr that is not finite, a weight that is not finite and > 0;
 *   CODETR_E_TOO_LARGE for V > CODETR_TTA_MAX_VIEWS or V * Q > CODETR_WBF_MAX_CANDIDATES.  All checks run before any
 *   HIP call.
 */
#ifndef CODETR_WBF_H_
#define CODETR_WBF_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_WBF_ABI_VERSION 1
#define CODETR_WBF_MAX_CANDIDATES 4096
#define CODETR_WBF_CONF_AVG 0
#define CODETR_WBF_CONF_MAX 1

int codetr_wbf_abi_version(void);
int codetr_wbf_merge_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                         const int *count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask,
                         const float *width_dev, const float *weights_host, int conf_type, float iou_threshold,
                         float skip_box_thr, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                         int64_t *labels_out_dev, int *index_out_dev, int *count_out_dev, int *votes_out_dev);
int codetr_wbf_merge_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                          const int *count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask,
                          const float *width_dev, const float *weights_host, int conf_type, float iou_threshold,
                          float skip_box_thr, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                          int64_t *labels_out_dev, int *index_out_dev, int *count_out_dev, int *votes_out_dev);
int codetr_wbf_merge_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                         const int *count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask,
                         const float *width_dev, const float *weights_host, int conf_type, float iou_threshold,
                         float skip_box_thr, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                         int64_t *labels_out_dev, int *index_out_dev, int *count_out_dev, int *votes_out_dev);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_WBF_H_ */
