/* codetr_redact.h -- companion header of codetr_hip.h: redaction of detected regions.  The pixels under the detections of
 * selected classes are made unrecognisable -- pixelated, blurred or filled -- in place in the packed RGB images the
 * pre-processing kernels read, before anything is drawn on them or encoded from them.  Exported from the same
 * libcodetr_hip.so; versioned on its own (CODETR_HIP_ABI_VERSION and the other companion headers are as they were).
 * Error codes and the limits CODETR_PREPROCESS_BATCH_MAX / CODETR_DRAW_MAX_Q / CODETR_DRAW_MAX_SIDE are codetr_hip.h's.
 *
 * Beyond the reference (its Inferencer draws, it does not redact).  The rule below is this library's own: "blur" is a box
 * filter over fixed cells followed by a tent (bilinear) reconstruction, NOT a Gaussian and not cv2.blur; parity with
 * OpenCV's blur is unpinned (cv2 is not part of this build).  Limits: a redaction is only as good as the detections -- a
 * missed object stays visible; the cells are anchored at the image's pixel (0, 0), so "pixelate" and "blur" of one
 * object change as it moves across the grid; a small cell on a large face may stay recognisable.
 *
 * The rule is exact: integers, and fp32 with one rounding per operation and no contraction, so that a restatement
 * (tests/redact_ref.py) reproduces every byte.
 *
 * Selection.  Row j of image n is redacted iff
 *     j < clamp(count[n], 0, Q);
 *     its score widened to fp32 is > score_thr (strict; a NaN score fails);
 *     its label is selected: select_dev is NULL, or 0 <= label < C and select_dev[label] != 0;
 *     its four coordinates (widened to fp32 exactly) are finite.
 * Region of a redacted row (x1, y1, x2, y2):
 *     each coordinate is clamped in fp32 to [-16384, 16383]:  v = fminf(fmaxf(v, -16384.0f), 16383.0f);
 *     w = x2 - x1;  h = y2 - y1;  ex = expand * w;  ey = expand * h      (each ONE fp32 operation with one rounding; the
 *                                                                         product and the sums below are never fused)
 *     a1 = x1 - ex;  a2 = x2 + ex;  b1 = y1 - ey;  b2 = y2 + ey,  each clamped to the same range;
 *     X1 = (int)floorf(a1);  X2 = (int)ceilf(a2) - 1;  Y1 = (int)floorf(b1);  Y2 = (int)ceilf(b2) - 1;
 *     the region exists iff X2 >= X1 and Y2 >= Y1.
 *   shape CODETR_REDACT_BOX: the pixels (x, y) with X1 <= x <= X2 and Y1 <= y <= Y2.
 *   shape CODETR_REDACT_ELLIPSE: those pixels of the rectangle with, Ww = X2 - X1 + 1 and Hh = Y2 - Y1 + 1,
 *     ((2x + 1 - X1 - X2 - 1) * Hh)^2 + ((2y + 1 - Y1 - Y2 - 1) * Ww)^2 <= (Ww * Hh)^2     in int64.
 *     The test is applied only inside the rectangle, where |2x - X1 - X2| < Ww and |2y - Y1 - Y2| < Hh; Ww, Hh <= 2^15, so
 *     no term exceeds 2^60.
 *   A pixel is MASKED when the region of any redacted row of its image holds it; everything is clipped to the image.
 * Cells.  The image is cut into cell x cell cells anchored at pixel (0, 0): cell (i, k) holds the pixels
 *   cell * i <= x < min(cell * (i + 1), W), cell * k <= y < min(cell * (k + 1), H) (edge cells are clipped).  The mean of
 *   a cell is, per channel, (sum + n / 2) / n over its n pixels in integer division -- over the image as it was BEFORE
 *   the call, never over a pixel this call has written.
 * Modes.  A masked pixel (x, y) becomes
 *   CODETR_REDACT_FILL      the three bytes of fill_rgb (0xRRGGBB);
 *   CODETR_REDACT_PIXELATE  the mean of its cell;
 *   CODETR_REDACT_BLUR      the bilinear interpolation of the four nearest cell means taken at the nominal cell centres
 *                           cell * i + cell / 2:  with c = cell and u = 2x + 1 - c,  i0 = floor(u / 2c) (towards minus
 *                           infinity),  fx = u - 2c * i0;  the columns are i0 and i0 + 1, each clamped to the cell grid
 *                           [0, ceil(W / c) - 1], with the weights wx = 2c - fx and fx; y likewise (k0, fy, wy);
 *                           per channel  (sum over the four of wx * wy * mean + 2 c^2) >> (2 log2 c + 2).
 *   An unmasked pixel is never written.  Overlapping regions give the same result in any order: only original values are
 *   read.  A constant image is a fixed point of PIXELATE and BLUR.
 *
 * codetr_redact_detections_{f16,bf16,f32}: in place, on `stream`, no host synchronisation (csrc/redact.hip: one workgroup
 *   per 64 x 64-pixel tile, a multiple of every cell, so a workgroup owns whole cells).  FILL and PIXELATE are one launch.
 *   BLUR is two: the first writes the means of the cells of every tile that a region grown by one cell reaches into
 *   work_dev, the second reads only work_dev and writes the masked pixels, so no workgroup reads a pixel that another may
 *   have written.  A tile that no region reaches returns before it touches a pixel.
 *     buf_dev, buf_bytes   the flat buffer of packed RGB HWC images; no alignment is assumed of it or of the offsets
 *     images_host          [N, 3] int64: byte offset, H, W of every image; 1 <= H, W <= CODETR_DRAW_MAX_SIDE; two images
 *                          may not share a byte
 *     boxes_dev            [N, Q, 4] of the element type, image pixels;  scores_dev [N, Q];  labels_dev [N, Q] int64;
 *                          count_dev [N] int32
 *     select_dev, C        [C] bytes, 1 = redact this label; NULL (then C is ignored) = every label
 *     mode, shape, cell    CODETR_REDACT_*; cell in {4, 8, 16, 32, 64}
 *     score_thr, expand    not NaN; expand in [0, 1]
 *     fill_rgb             0xRRGGBB
 *     work_dev, work_bytes BLUR only (may be NULL / 0 otherwise): at least codetr_redact_work_bytes(N, images_host, cell)
 *                          bytes of device scratch, 4-byte aligned (this library allocates nothing).  It holds one uint32
 *                          (R | G << 8 | B << 16) per cell, image after image.
 *   CODETR_E_BADARG for a null pointer, N, Q or buf_bytes <= 0, C <= 0 with a table, a row outside the buffer or with H
 *   or W < 1, overlapping images, a mode, shape or cell outside its set, a NaN score_thr, expand outside [0, 1],
 *   fill_rgb > 0xffffff, a missing, misaligned or too small workspace; CODETR_E_TOO_LARGE for
 *   N > CODETR_PREPROCESS_BATCH_MAX, Q > CODETR_DRAW_MAX_Q, C > 65536, a side above CODETR_DRAW_MAX_SIDE.  All checks run
 *   before any HIP call.
 * codetr_redact_work_bytes: host only; 4 * the sum over the images of ceil(H / cell) * ceil(W / cell), or a negative
 *   CODETR_E_* code by the same checks of N, the rows' H and W, and cell (the offsets are not read).
 */
#ifndef CODETR_REDACT_H_
#define CODETR_REDACT_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_REDACT_ABI_VERSION 1
#define CODETR_REDACT_PIXELATE 0
#define CODETR_REDACT_BLUR 1
#define CODETR_REDACT_FILL 2
#define CODETR_REDACT_BOX 0
#define CODETR_REDACT_ELLIPSE 1
#define CODETR_REDACT_TILE 64

int codetr_redact_abi_version(void);
int64_t codetr_redact_work_bytes(int64_t N, const int64_t *images_host, int64_t cell);
int codetr_redact_detections_f16(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                                 const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                                 const int *count_dev, int64_t Q, const unsigned char *select_dev, int64_t C, int mode,
                                 int shape, int cell, float score_thr, float expand, uint32_t fill_rgb, void *work_dev,
                                 int64_t work_bytes);
int codetr_redact_detections_bf16(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                                  const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                                  const int *count_dev, int64_t Q, const unsigned char *select_dev, int64_t C, int mode,
                                  int shape, int cell, float score_thr, float expand, uint32_t fill_rgb, void *work_dev,
                                  int64_t work_bytes);
int codetr_redact_detections_f32(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                                 const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                                 const int *count_dev, int64_t Q, const unsigned char *select_dev, int64_t C, int mode,
                                 int shape, int cell, float score_thr, float expand, uint32_t fill_rgb, void *work_dev,
                                 int64_t work_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_REDACT_H_ */
