/* codetr_crops.h -- companion header of codetr_hip.h: crops of detected objects for a second-stage model.  The regions
 * under the detections of selected classes are resampled, with antialiasing, to one fixed size: uint8 HWC crops and,
 * when asked, the same crops normalised as CHW tensors.  The images are only read.  Exported from the same
 * libcodetr_hip.so; versioned on its own (CODETR_HIP_ABI_VERSION and the other companion headers are as they were).
 * Error codes and the limits CODETR_PREPROCESS_BATCH_MAX / CODETR_DRAW_MAX_Q / CODETR_DRAW_MAX_SIDE are codetr_hip.h's.
 *
 * Beyond the reference (its Inferencer hands out detections, not objects).  Limits: nothing here is learned -- the crops
 * feed a network the caller brings; boxes stay axis-aligned (no rotation, no perspective); parity with cv2.resize
 * (INTER_AREA or INTER_LINEAR) is unpinned (cv2 is not part of this build).  The filter is the antialiased triangle
 * filter of Pillow's resize(size, BILINEAR, box=region) and torchvision's antialias=True, but not Pillow's arithmetic:
 * Pillow rounds its coefficients to 22 fractional bits and its horizontal pass to 8 bits; this rule keeps integer
 * weights exactly and the horizontal pass to 8 + 8 bits.  And not Pillow's footprint: with box= inside a larger image
 * Pillow lets the outermost taps read the image beyond the box, this rule reads the region alone.  Measured on the cases
 * of tests/crops_ref.py (Pillow 12.2): against resize(size, BILINEAR, box=region) the largest difference is 79 (a
 * one-pixel region: Pillow blends its neighbours in); against the same call on the region cut out first the largest
 * difference is 1, on 0 to 20 % of a case's bytes.
 *
 * The rule is exact: integers, and fp32 with one rounding per operation for the region and the tensor form, so that a
 * restatement (tests/crops_ref.py) reproduces every byte.
 *
 * Selection.  Row j of image n is a candidate iff
 *     j < clamp(count[n], 0, Q);
 *     its score widened to fp32 is >= score_thr (a NaN score fails);
 *     its label is selected: select_dev is NULL, or 0 <= label < C and select_dev[label] != 0;
 *     its four coordinates (widened to fp32 exactly) are finite;
 *     its region, below, is not empty.
 *   The candidates are taken in row order; the first max_per_img fill the slots 0, 1, ... of the image, and
 *   counts[n] = min(candidates, max_per_img).
 * Region.  (X1, Y1, X2, Y2) by the region rule of codetr_redact.h (clamp to [-16384, 16383], grow by expand, floor and
 *   ceil - 1; one implementation serves both), then clipped to the H x W image as a half-open rectangle:
 *     x0 = max(X1, 0);  x1 = min(X2 + 1, W);  y0 = max(Y1, 0);  y1 = min(Y2 + 1, H);
 *   empty iff the redaction's region does not exist or x1 <= x0 or y1 <= y0.  Rw = x1 - x0, Rh = y1 - y0.
 * Fit.  The region is mapped onto the inner rectangle [ox, ox + iw) x [oy, oy + ih) of the out_w x out_h output:
 *   CODETR_CROPS_STRETCH  ox = oy = 0, iw = out_w, ih = out_h;
 *   CODETR_CROPS_PAD      the largest centred rectangle of the region's aspect ratio, in integers:
 *                           if Rw * out_h >= Rh * out_w:  iw = out_w,  ih = clamp((2 Rh out_w + Rw) / (2 Rw), 1, out_h)
 *                           else:                         ih = out_h,  iw = clamp((2 Rw out_h + Rh) / (2 Rh), 1, out_w)
 *                         (integer division: round half up);  ox = (out_w - iw) / 2,  oy = (out_h - ih) / 2.
 *                         Every output pixel outside the inner rectangle is pad_rgb (0xRRGGBB).
 * Resampling.  Along an axis with region length R and inner length n, in units of 1 / (2n) source pixel:
 *     S = 2 max(n, R);   wt(j, s) = max(0, S - |(2s + 1) n - (2j + 1) R|)   for the source pixels 0 <= s < R;
 *     Nrm(j) = the sum of wt(j, s) over s   (> 0: the pixel under the sample centre always has a positive weight).
 *   This is the triangle filter of half-width max(1, R / n) about the centre (j + 1/2) R / n, normalised over the taps
 *   inside the region: pixels outside the region are never read, even where the image has them.
 *   Horizontal pass first, per source row y, inner column i and channel:
 *     hs = the sum over s of wt_x(i, s) * pixel(y0 + y, x0 + s);
 *     t(y, i) = (hs * 256 + Nrm_x(i) / 2) / Nrm_x(i)            (integer division: the row value in 8.8 fixed point,
 *                                                                rounded half up; 0 <= t <= 65280)
 *   then the vertical pass and ONE final rounding:
 *     vs = the sum over y of wt_y(j, y) * t(y, i);   D = 256 * Nrm_y(j);   out(oy + j, ox + i) = (vs + D / 2) / D.
 *   Accuracy: the final rounding costs at most 1/2 LSB; the rounding of t costs at most 1/512 LSB per row and the
 *   normalised vertical weights sum to one, so |out - the unrounded filter| <= 1/2 + 1/512 LSB.  A region resampled to
 *   its own size is copied exactly (one tap of weight S); a constant image gives that constant.
 *   Widths, at the limits R <= 16384, n >= 1:  |(2s + 1) n|, |(2j + 1) R| <= 2^24 (int32);  Nrm <= S^2 / (2n) + S
 *   < 2^30 (uint32);  hs <= 255 Nrm < 2^38, hs * 256 + Nrm / 2 < 2^47, vs <= 65280 Nrm_y < 2^46, D < 2^38 (uint64).
 * Tensor form (tensor_type != CODETR_CROPS_TENSOR_NONE): element (c, row, col) of a slot is, from the uint8 crop value v,
 *     ((float)v - mean[c]) / std[c]     one fp32 subtract and one IEEE fp32 divide, as the pre-processing kernels have it,
 *   stored as fp32, or rounded once to nearest even to fp16 / bf16.
 *
 * codetr_crop_detections_{f16,bf16,f32} (the suffix is the detections' element type): on `stream`, no host
 * synchronisation, two launches (csrc/crops.hip): a selection pass, one workgroup per image, that writes table_dev and
 * counts_dev, and the resampling kernel over slots x bands of output rows; workgroups of slots beyond counts[n] return
 * at once and those slots are left unwritten.
 *     buf_dev, buf_bytes   the flat buffer of packed RGB HWC images, read only; no alignment is assumed
 *     images_host          [N, 3] int64: byte offset, H, W of every image; 1 <= H, W <= CODETR_DRAW_MAX_SIDE (rows may
 *                          share bytes: nothing is written there)
 *     boxes_dev            [N, Q, 4] of the element type, image pixels;  scores_dev [N, Q];  labels_dev [N, Q] int64;
 *                          count_dev [N] int32
 *     select_dev, C        [C] bytes, 1 = crop this label; NULL (then C is ignored) = every label
 *     out_w, out_h         CODETR_CROPS_MIN_SIDE .. CODETR_CROPS_MAX_SIDE each
 *     max_per_img          M, 1 .. CODETR_CROPS_MAX_PER_IMG
 *     fit                  CODETR_CROPS_STRETCH / CODETR_CROPS_PAD;  pad_rgb 0xRRGGBB
 *     score_thr, expand    not NaN; expand in [0, 1]
 *     crops_dev            [N, M, out_h, out_w, 3] uint8;  counts_dev [N] int32
 *     table_dev            [N, M, CODETR_CROPS_TABLE_INTS] int32, 4-byte aligned: per slot the row index, x0, y0, x1, y1,
 *                          ox, oy, iw, ih and three unused words (this library allocates nothing)
 *     tensor_dev, tensor_type, mean_host, std_host
 *                          [N, M, 3, out_h, out_w] of CODETR_CROPS_TENSOR_F32 / _F16 / _BF16 with three means and three
 *                          non-zero divisors; CODETR_CROPS_TENSOR_NONE: all three may be NULL
 *   CODETR_E_BADARG for a null pointer, N, Q or buf_bytes <= 0, C <= 0 with a table, an image outside the buffer or with
 *   H or W < 1, out_w, out_h or max_per_img below its range, a fit or tensor_type outside its set, a NaN score_thr,
 *   expand outside [0, 1], pad_rgb > 0xffffff, a misaligned table, a tensor without its pointers or not aligned to its
 *   element's size, a NaN mean, a divisor that is zero or NaN; CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX,
 *   Q > CODETR_DRAW_MAX_Q, C > 65536, a side above CODETR_DRAW_MAX_SIDE, out_w or out_h above CODETR_CROPS_MAX_SIDE,
 *   max_per_img above CODETR_CROPS_MAX_PER_IMG.
 *   All checks run before any HIP call.
 */
#ifndef CODETR_CROPS_H_
#define CODETR_CROPS_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_CROPS_ABI_VERSION 1
#define CODETR_CROPS_STRETCH 0
#define CODETR_CROPS_PAD 1
#define CODETR_CROPS_MIN_SIDE 8
#define CODETR_CROPS_MAX_SIDE 512
#define CODETR_CROPS_MAX_PER_IMG 256
#define CODETR_CROPS_TABLE_INTS 12
#define CODETR_CROPS_TENSOR_NONE 0
#define CODETR_CROPS_TENSOR_F32 1
#define CODETR_CROPS_TENSOR_F16 2
#define CODETR_CROPS_TENSOR_BF16 3

int codetr_crops_abi_version(void);
int codetr_crop_detections_f16(void *stream, const void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                               const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                               const int *count_dev, int64_t Q, const unsigned char *select_dev, int64_t C, int out_w,
                               int out_h, int max_per_img, int fit, float score_thr, float expand, uint32_t pad_rgb,
                               void *crops_dev, int *counts_dev, int *table_dev, void *tensor_dev, int tensor_type,
                               const float *mean_host, const float *std_host);
int codetr_crop_detections_bf16(void *stream, const void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                                const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                                const int *count_dev, int64_t Q, const unsigned char *select_dev, int64_t C, int out_w,
                                int out_h, int max_per_img, int fit, float score_thr, float expand, uint32_t pad_rgb,
                                void *crops_dev, int *counts_dev, int *table_dev, void *tensor_dev, int tensor_type,
                                const float *mean_host, const float *std_host);
int codetr_crop_detections_f32(void *stream, const void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                               const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                               const int *count_dev, int64_t Q, const unsigned char *select_dev, int64_t C, int out_w,
                               int out_h, int max_per_img, int fit, float score_thr, float expand, uint32_t pad_rgb,
                               void *crops_dev, int *counts_dev, int *table_dev, void *tensor_dev, int tensor_type,
                               const float *mean_host, const float *std_host);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_CROPS_H_ */
