/* codetr_motion.h -- companion header of codetr_hip.h: the global image motion between the consecutive frames of a
 * stream, estimated on the GPU from the packed RGB images the pre-processing kernels read, and the tracker that shifts its
 * predicted track centres by it before association ("camera-motion compensation", the GMC step of BoT-SORT and the later
 * trackers of the ByteTrack family).  Exported from the same libcodetr_hip.so; versioned on its own (a self-contained
 * addition does not touch CODETR_HIP_ABI_VERSION, and codetr_assign.h is as it was).  Error codes and the limits
 * CODETR_PREPROCESS_BATCH_MAX / CODETR_FRAME_MAX_SIDE are codetr_hip.h's.
 *
 * Beyond the reference (its Inferencer has no tracker).  Deviations from BoT-SORT's estimate (sparse optical flow and a
 * RANSAC affine fit, in OpenCV): the model is a TRANSLATION only -- zoom and roll are not modelled; blocks that lie under
 * detections are not masked out -- the median outvotes them; parity with that estimate is unpinned (OpenCV is not
 * installed where this was built).  The reach is `search * k` source pixels per frame (k below): 96 px at 1920 x 1080 with
 * the defaults, 192 px with search = 16; a larger pan gives an arbitrary or an invalid motion.
 *
 * The rule is integer arithmetic except for one final fp32 division per axis, so that a restatement (tests/motion_ref.py)
 * reproduces every output bit.  All divisions of integers below are of non-negative operands (truncation) unless stated.
 *
 * Settings (settings_host, 4 ints): grid G in 32 .. 160 (default 160), search R in 1 .. 16 (default 8), texture in
 *   0 .. 65535 (default 2), min_blocks in 1 .. 100 (default 4).  The block is 16 x 16 cells, fixed.
 * Thumbnail of an H x W packed RGB image: k = max(1, ceil(max(H, W) / G)), th = H / k, tw = W / k.  Pixels beyond th * k
 *   rows or tw * k columns take no part.  gray = (77 R + 150 G + 29 B + 128) >> 8 per pixel; a cell is
 *   (the sum of its k * k grays + (k * k) / 2) / (k * k), one byte.  Rows at pitch tw.
 * Blocks: nbx = max(0, (tw - 2 R) / 16), nby = max(0, (th - 2 R) / 16); block b = by * nbx + bx has its origin at row
 *   R + 16 by, column R + 16 bx of the PREVIOUS thumbnail P.  It is textured iff the sum over its 16 x 16 cells of
 *   |P[y][x] - P[y][x + 1]| (the 15 pairs of every row) plus |P[y][x] - P[y + 1][x]| (the 15 pairs of every column) is
 *   >= texture * 256.
 * Vote of a textured block: S(dy, dx) = the sum over the block of |P[y][x] - C[y + dy][x + dx]| for every (dy, dx) in
 *   [-R, R]^2, C the current thumbnail.  The best displacement has the least S; ties go to the least dy * dy + dx * dx,
 *   then the lowest dy, then the lowest dx.  Sub-cell step of an axis, only where both neighbours of the best along that
 *   axis lie inside the search square (0 otherwise): den = S(-1) - 2 S(0) + S(+1); if den > 0 the step is
 *   clamp(floor((16 (S(-1) - S(+1)) + den) / (2 den)), -8, 8) -- a FLOOR division, the numerator may be negative --
 *   otherwise 0.  The vote is (vx, vy) = (16 dx + step_x, 16 dy + step_y), in sixteenths of a cell.
 * Frame motion: n = the number of textured blocks; n < min_blocks: invalid.  (mx, my) = the per-axis lower median of the
 *   votes: the element at index (n - 1) / 2 of the ascending sort.  A block agrees iff |vx - mx| <= 16 and
 *   |vy - my| <= 16; c = the number of agreeing blocks; 2 c < n: invalid.  Otherwise
 *   dx = (float)(sum_x * k) / (float)(16 * c), dy likewise, sum over the agreeing blocks' votes (int32; one int -> fp32
 *   conversion of each operand, round to nearest even, and one IEEE fp32 division).
 *   Meaning: scene content at p in the previous frame appears at p + (dx, dy) in this frame, in source pixels.
 * A frame is invalid (dx = dy = 0, valid = 0) when it is the first of its stream, when its predecessor had another H, W
 *   or k (k: the grid setting changed between calls), when it has no blocks, or when one of the two conditions above
 *   fails.
 * State of a stream, on the device, all zero when fresh: int32 {have, H, W, k}, then 160 * 160 thumbnail bytes (rows at
 *   pitch tw, the bytes beyond th * tw zero).  codetr_motion_state_bytes() = 16 + 25600.
 *
 * Choices of this library beyond the rule as first proposed: the entry point takes the buffer's size (every row is
 *   bounds-checked) and a scratch buffer of the caller's (the library allocates nothing); a predecessor counts only with
 *   the same k as well as the same H and W; the state's bytes behind the thumbnail are zeroed, so a state is a function
 *   of the stream's last frame alone; diag reports k and the block count of every row, usable predecessor or not.
 *
 * codetr_motion_estimate_u8: N <= CODETR_PREPROCESS_BATCH_MAX images of one buffer in three launches on `stream`
 *   (csrc/motion.hip: thumbnails; one workgroup per (row, block) for the votes; one per row for the motion, and for a
 *   stream's last row the state, which the second launch still reads).  No host synchronisation.
 *     src_dev, src_bytes  the flat buffer of packed RGB HWC images
 *     rows_host           [N, 3] int64: byte offset, H, W of every image; 1 <= H, W <= CODETR_FRAME_MAX_SIDE
 *     stream_of_row_host  [N] in [0, S): the rows of a stream are its consecutive frames in row order; the predecessor
 *                         of a stream's first row in the launch is the state's thumbnail
 *     state_dev           [S] states as above; after the call a stream with rows holds its last row, others are untouched
 *     work_dev            codetr_motion_work_bytes(N) bytes of device scratch, 4-byte aligned (this library allocates
 *                         nothing: the N thumbnails and the blocks' votes live here between the launches)
 *     motion_out_dev      [N, 4] float32: dx, dy, valid (1.0 / 0.0), 0
 *     diag_out_dev        [N, 4] int32: k, nbx * nby, textured n, agreeing c.  n is 0 without a usable predecessor; c is 0
 *                         there and where n < min_blocks.
 *   CODETR_E_BADARG for a null pointer, N or S <= 0, a row outside the buffer or with H or W < 1, a stream outside
 *   [0, S), a setting outside its range, work_bytes too small; CODETR_E_TOO_LARGE for N, H or W above the limits.  All
 *   checks run before any HIP call.
 *
 * codetr_track_update3_{f16,bf16,f32}: codetr_track_update2_* (codetr_assign.h) with one more argument:
 *     motion_dev  [N, 4] float32 on the device as motion_out_dev above, or NULL.
 *   In step 2 of codetr_hip.h's "Tracking", after m[0] = m[0] + m[maxT] of cx and cy of a live track and before its
 *   predicted box: cx = cx + dx, cy = cy + dy (one fp32 addition each, stored in the state), iff the row's valid == 1.0f
 *   and dx and dy are both finite.  Velocities, covariances, steps 1 and 3 to 9 and the state layout are unchanged.
 *   NULL gives codetr_track_update2_*'s ids and state bytes.
 */
#ifndef CODETR_MOTION_H_
#define CODETR_MOTION_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_MOTION_ABI_VERSION 1
#define CODETR_MOTION_GRID_MIN 32
#define CODETR_MOTION_GRID_MAX 160
#define CODETR_MOTION_BLOCK 16
#define CODETR_MOTION_SEARCH_MAX 16
#define CODETR_MOTION_TEXTURE_MAX 65535
#define CODETR_MOTION_MAX_BLOCKS 100

int codetr_motion_abi_version(void);
int64_t codetr_motion_state_bytes(void);
int64_t codetr_motion_work_bytes(int64_t N);
int codetr_motion_estimate_u8(void *stream, const void *src_dev, int64_t src_bytes, int64_t N, const int64_t *rows_host,
                              const int *stream_of_row_host, int64_t S, void *state_dev, const int *settings_host,
                              void *work_dev, int64_t work_bytes, float *motion_out_dev, int *diag_out_dev);
int codetr_track_update3_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                             const float *motion_dev);
int codetr_track_update3_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                              const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                              void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                              int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                              const float *motion_dev);
int codetr_track_update3_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                             const float *motion_dev);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_MOTION_H_ */
