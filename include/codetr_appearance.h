/* codetr_appearance.h -- companion header of codetr_hip.h: an appearance cue for the tracker.  A colour descriptor of
 * every detection, gathered on the GPU from the packed RGB images the pre-processing kernels read, an appearance kept per
 * track, and the tracker that adds their similarity to the overlap in its first two associations (the second ingredient of
 * BoT-SORT beside the camera motion of codetr_motion.h).  Exported from the same libcodetr_hip.so; versioned on its own
 * (CODETR_HIP_ABI_VERSION and the other companion headers are as they were).  Error codes and the limits
 * CODETR_PREPROCESS_BATCH_MAX / CODETR_POSTPROCESS_MAX_Q / CODETR_FRAME_MAX_SIDE / CODETR_TRACK_MAX_TRACKS are
 * codetr_hip.h's.
 *
 * Beyond the reference (its Inferencer has no tracker).  Limits: the descriptor is a histogram over HARD 2-bit colour
 * bins (a colour near a bin edge falls to either side); it has no spatial layout beyond two stripes (upper and lower
 * half); NOTHING is learned (BoT-SORT uses a FastReID network: there are no weights here); an object hidden under another
 * has the other's colours; parity with BoT-SORT / FastReID is unpinned.  Deviation from BoT-SORT's fusion, on purpose:
 * it takes the minimum of the overlap distance and the appearance distance; here the similarity is ADDED to the overlap
 * value (below), which keeps the overlap's order among objects that look alike and lets a lost track inside the gate match
 * on appearance alone (v = 0, value = s).
 *
 * The rule is exact: integers, and fp32 with one rounding per operation and no contraction, so that a restatement
 * (tests/appearance_ref.py) reproduces every bit.
 *
 * Descriptor of a detection: 128 uint16, two stripes of 64 colour bins, from the packed RGB HWC image (H x W) of its row.
 *   The box (x1, y1, x2, y2) is widened to fp32 exactly; w = x2 - x1, h = y2 - y1.  Row j of image n takes part iff
 *   j < clamp(count[n], 0, Q), all four coordinates are finite, w > 0 and h > 0 (step 1 of "Tracking" without the score);
 *   any other row is 128 zeros.  16 columns x 32 rows of samples over the inner three quarters of the box:
 *     u_i = (float)(6 i + 19) / 128.0f, i in 0..15;   v_j = (float)(6 j + 35) / 256.0f, j in 0..31   (both exact)
 *     x = x1 + w * u_i;  y = y1 + h * v_j                       (one rounding per operation)
 *     px = (int)fminf(fmaxf(floorf(x), 0.0f), (float)(W - 1)), py likewise with H
 *   (fmaxf / fminf return the non-NaN operand, so an overflowed coordinate lands on an edge pixel.)  Sample (i, j) adds 1
 *   to bin (j / 16) * 64 + (R >> 6) * 16 + (G >> 6) * 4 + (B >> 6) of the pixel (py, px).  Every stripe of a participating
 *   row sums to 256.
 * Appearance of a track: g[128] uint16 in sixteenths, all 0 for a free slot.  A stream's appearance state is uint16
 *   [T][128]: codetr_appearance_state_bytes(T) = 256 T, zero-filled when fresh; a buffer of its own (the tracker state of
 *   codetr_hip.h keeps its layout).
 * Similarity of track t and candidate j: I = sum over k of min(g[k], 16 * d[k]) in 32-bit integers (in [0, 8192] for a
 *   descriptor of this header), s = (float)I / 8192.0f (exact).
 * Settings (app_settings_host, 3 floats): appearance_thr (default 0.75: BoT-SORT's appearance_thresh 0.25 as a distance,
 *   as recalled), proximity_thr (default 0.5: BoT-SORT's proximity_thresh, as recalled), reid_gate (default 1.5: this
 *   library's own).  All finite, the thresholds in [0, 1], reid_gate >= 0.
 * Association: steps 1 to 9 of "Tracking" in codetr_hip.h (or codetr_assign.h's optimal association) and the motion of
 *   codetr_track_update4_* as they are, except:
 *   Matches A and B (the `high` candidates), pair (track t, candidate j):
 *     v = the value as it is: iou, or iou * score (a NaN v leaves the pair ineligible);
 *     near = iou >= proximity_thr;
 *     lost = t is confirmed and last[t] != f - 1 (a tentative track, hence any track of Match B, is never lost);
 *     for a lost track with reid_gate > 0, with the track's predicted mean after the camera motion (cx, cy, a, hh) and the
 *     candidate's centre (ccx, ccy) = ((x1 + x2) * 0.5f, (y1 + y2) * 0.5f) as in "A detection's measurement":
 *       dx = ccx - cx; dy = ccy - cy; d2 = dx * dx + dy * dy;
 *       wt = a * hh; r2 = (reid_gate * reid_gate) * (wt * wt + hh * hh);
 *       near = near || d2 <= r2;
 *     value = v + s when near && s >= appearance_thr, else value = v.
 *     Eligibility (labels equal, value >= the phase's threshold), ties, the greedy order and the optimal gain
 *     1 + (int)(min(value - thr, 2) * 2^20) are unchanged, now taken of `value`.
 *   Match C: unchanged, plain IoU.
 *   Step 6: a track matched to a `high` candidate (Match A or B) updates its appearance: if all 128 g are 0,
 *     g[k] = 16 d[k]; otherwise g[k] = (7 g[k] + 16 d[k] + 4) >> 3 (32-bit, stored as uint16).  A match in C leaves g.
 *   Step 7: a freed slot's g is zeroed.   Step 8: a started track takes g[k] = 16 d[k].
 *   A live track whose g is all zero (a stream that switched entry points) has s = 0 and adopts the first `high` match's
 *   descriptor.
 *
 * codetr_appearance_describe_{f16,bf16,f32}: one launch on `stream` (csrc/appearance.hip: a wave per detection), no host
 *   synchronisation; every element of desc_out_dev is written.
 *     src_dev, src_bytes  the flat buffer of packed RGB HWC images
 *     rows_host           [N, 3] int64: byte offset, H, W of every image; 1 <= H, W <= CODETR_FRAME_MAX_SIDE
 *     boxes_dev           [N, Q, 4] of the element type, source pixels;  count_dev [N] int32
 *     desc_out_dev        [N, Q, 128] uint16
 *   CODETR_E_BADARG for a null pointer, N, Q or src_bytes <= 0, a row outside the buffer or with H or W < 1;
 *   CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX, Q > CODETR_POSTPROCESS_MAX_Q, a side above the limit.  All
 *   checks run before any HIP call.
 *
 * codetr_track_update5_{f16,bf16,f32}: codetr_track_update4_*'s arguments (motion_dev: the [N, 8] rows, or NULL), then
 *     desc_dev           [N, Q, 128] uint16 as desc_out_dev above, 16-byte aligned, or NULL
 *     app_state_dev      [S] appearance states of max_tracks slots, 4-byte aligned (may be NULL with desc_dev NULL)
 *     app_settings_host  the 3 floats above (may be NULL with desc_dev NULL)
 *     work_dev, work_bytes  codetr_appearance_work_bytes(S, max_tracks, Q) bytes of device scratch, 4-byte aligned (this
 *                        library allocates nothing; may be NULL with desc_dev NULL).  It holds one fp32 per (stream, slot,
 *                        candidate): the addend of the pair (s where it is added, 0 elsewhere), written by a pre-pass of
 *                        every frame (a wave per live track) and looked up by the associations.
 *   One launch (track_kernel's form with the cue, csrc/track.hip), one workgroup per stream; the appearance state stays in
 *   global memory.  With desc_dev NULL the ids and state bytes are codetr_track_update4_*'s and no appearance state is
 *   touched.  CODETR_E_BADARG also for a setting outside its range, a missing or misaligned buffer, work_bytes too small.
 */
#ifndef CODETR_APPEARANCE_H_
#define CODETR_APPEARANCE_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_APPEARANCE_ABI_VERSION 1
#define CODETR_APPEARANCE_BINS 128
#define CODETR_APPEARANCE_COLS 16
#define CODETR_APPEARANCE_ROWS 32

int codetr_appearance_abi_version(void);
int64_t codetr_appearance_state_bytes(int64_t max_tracks);
int64_t codetr_appearance_work_bytes(int64_t S, int64_t max_tracks, int64_t Q);
int codetr_appearance_describe_f16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *rows_host, const void *boxes_dev, const int *count_dev, int64_t Q,
                                   uint16_t *desc_out_dev);
int codetr_appearance_describe_bf16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                    const int64_t *rows_host, const void *boxes_dev, const int *count_dev, int64_t Q,
                                    uint16_t *desc_out_dev);
int codetr_appearance_describe_f32(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *rows_host, const void *boxes_dev, const int *count_dev, int64_t Q,
                                   uint16_t *desc_out_dev);
int codetr_track_update5_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                             const float *motion_dev, const uint16_t *desc_dev, void *app_state_dev,
                             const float *app_settings_host, void *work_dev, int64_t work_bytes);
int codetr_track_update5_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                              const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                              void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                              int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                              const float *motion_dev, const uint16_t *desc_dev, void *app_state_dev,
                              const float *app_settings_host, void *work_dev, int64_t work_bytes);
int codetr_track_update5_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                             const float *motion_dev, const uint16_t *desc_dev, void *app_state_dev,
                             const float *app_settings_host, void *work_dev, int64_t work_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_APPEARANCE_H_ */
