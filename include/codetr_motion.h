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
/* Version 2: the SIMILARITY model (zoom and roll as well as the pan), fitted to the same block votes; everything above is
 * as it was, and what it says of the translation model holds for codetr_motion_estimate_u8 and codetr_track_update3_*.
 *
 * Limits of the similarity model: shear and perspective are not modelled; the reach is the translation rule's per block
 * (`search` cells), which at the corners of a 160-cell thumbnail with search = 8 is roughly 5 % of zoom or 0.05 rad of roll
 * per frame (8 cells over the 80 x 80 half-diagonal's 113 cells leave 7 %, less the pan; derived from the geometry, not
 * measured); the tracker's boxes stay axis-aligned (a roll turns the centres, not the boxes); parity with OpenCV's
 * estimateAffinePartial2D is unpinned.
 *
 * The rule.  Thumbnails, blocks, the texture test and the votes are the rule above.  All of the following is exact integer
 * arithmetic up to the conversions and divisions of "Output".
 * Points: block b = (bx, by) has the centre P_b = (16 (R + 16 bx + 8), 16 (R + 16 by + 8)) in sixteenths of a cell (cell i
 *   covers [i, i + 1)), and the image Q_b = P_b + (vx_b, vy_b).  The textured blocks, in ascending b, are numbered
 *   0 .. n - 1; i, j and m below are such numbers, g_i = (bx, by) of block i.
 * Hypotheses: every pair i < j with |D|^2 >= 4, D = g_j - g_i ("eligible").  For it d = P_j - P_i (= 256 D),
 *   e = Q_j - Q_i, dd = d.d, A = d.e, B = d_x e_y - d_y e_x.  Block m is an inlier of the pair iff both components of
 *       r = A u + B u_perp - dd w,    u = P_m - P_i,  u_perp = (-u_y, u_x),  w = Q_m - Q_i
 *   are at most 16 dd in absolute value (one cell, the translation rule's tolerance; i and j are inliers of their own pair:
 *   dd e = A d + B d_perp, so r = 0; r / dd is the pair's similarity applied to u, less w.  The sign of the B term is
 *   the one under which this holds: with - B u_perp, as the rule was first proposed, a pair's own j is no inlier of it
 *   under any roll).  d and u are multiples of 256: with D, U = u / 256, A' = D.e, B' = D_x e_y - D_y e_x, dd' = D.D the
 *   test is |A' U + B' U_perp - dd' w| <= 16 dd' per component.  Bound: block indices are 0 .. 9, |v| <= 264 per
 *   component, so |D|, |U| <= 9, |e|, |w| <= 2304 + 528, |A'|, |B'| <= 2 * 9 * 2832 < 2^16, dd' <= 162, and every term and
 *   sum of the reduced test is below 2 * 9 * 2^16 + 162 * 2832 < 2^21: int32 holds it (also when the test is taken as
 *   the difference of its value at block m and at block i from a common origin, as csrc/motion.hip takes it).
 *   The best pair has the most inliers c2; ties go to the lowest i, then the lowest j.
 * Validity: n >= min_blocks, at least one eligible pair, c2 >= min_blocks, 2 c2 >= n, and the refit's four conditions.
 * Refit over the best pair's inliers, int64 sums: sp = sum P, sq = sum Q, Sxx = c2 sum |P|^2 - |sp|^2,
 *   An = c2 sum P.Q - sp.sq, Bn = c2 sum (P_x Q_y - P_y Q_x) - (sp_x sq_y - sp_y sq_x).  Required: Sxx > 0, 2 An >= Sxx,
 *   An <= 2 Sxx, 2 |Bn| <= Sxx (the scale stays inside [0.5, 2]).
 * Output of a similarity row: [dx, dy, 1, 2, a, b, px, py].  Every integer operand is converted to fp32 once (round to
 *   nearest even), each output is one IEEE fp32 division:
 *     a = (float)An / (float)Sxx, b = (float)Bn / (float)Sxx,
 *     px = (float)(sp_x k) / (float)(16 c2), py likewise: the inliers' centroid in source pixels,
 *     dx = (float)((sq_x - sp_x) k) / (float)(16 c2), dy likewise: their mean displacement.
 *   Meaning: scene content at p in the previous frame appears at (px + dx, py + dy) + M (p - (px, py)) in this frame,
 *   M = [[a, -b], [b, a]].
 * Fallback: a row whose similarity is not valid holds the translation rule's result over all textured blocks:
 *   [dx, dy, 1, 1, 1, 0, 0, 0] with codetr_motion_estimate_u8's dx and dy (bit-equal) where that is valid, eight zeros
 *   otherwise.  The fourth float is the row's model: 2, 1 or 0.
 *
 * codetr_motion_estimate2_u8: codetr_motion_estimate_u8's arguments, checks and state (a stream may switch between the
 *   two from call to call), except
 *     work_dev, work_bytes  codetr_motion_work2_bytes(N) bytes, 4-byte aligned
 *     motion_out_dev        [N, 8] float32 as above
 *     diag_out_dev          [N, 8] int32: k, nbx * nby, textured n, the translation rule's agreeing c (as above), eligible
 *                           pairs, the best pair's inliers c2 (0 without an eligible pair), its i, its j (-1 without one).
 *                           The last four are of the search alone: min_blocks and the refit have no say in them.
 *   Five launches on `stream`, no host synchronisation: the three above (the third writes its row into the scratch, and
 *   the states), motion_sim_pairs_kernel (a row's pairs over the lanes of several workgroups, the votes in LDS; the best pair of
 *   each workgroup is one packed 64-bit maximum: count, ~i, ~j) and motion_sim_fit_kernel (one workgroup per row: the best of
 *   the workgroups' pairs, its inliers, the refit and the row).
 *
 * codetr_track_update4_{f16,bf16,f32}: codetr_track_update3_* with motion_dev [N, 8] float32 as motion_out_dev of
 *   codetr_motion_estimate2_u8, or NULL.  In step 2 of "Tracking", after m[0] = m[0] + m[maxT] of a live track and before
 *   its predicted box, by the row's model float:
 *     2.0f and a, b, px, py, dx, dy all finite -- fp32, one rounding per operation in the order written, no contraction:
 *       ux = cx - px; uy = cy - py;
 *       cx = (px + dx) + (a * ux - b * uy); cy = (py + dy) + (b * ux + a * uy);
 *       the velocities of cx and cy: (vx, vy) = (a * vx - b * vy, b * vx + a * vy);
 *       s = sqrt(a * a + b * b), correctly rounded; h = h * s; the velocity of h is multiplied by s too.
 *       The aspect ratio and all covariances stay.  (BoT-SORT transforms the covariance as well: this library's deviation.)
 *     1.0f and dx, dy finite -- codetr_track_update3_*'s two additions.
 *     anything else -- nothing is applied.
 *   NULL gives codetr_track_update2_*'s ids and state bytes.
 */
#ifndef CODETR_MOTION_H_
#define CODETR_MOTION_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_MOTION_ABI_VERSION 2
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

/* version 2 */
int64_t codetr_motion_work2_bytes(int64_t N);
int codetr_motion_estimate2_u8(void *stream, const void *src_dev, int64_t src_bytes, int64_t N, const int64_t *rows_host,
                               const int *stream_of_row_host, int64_t S, void *state_dev, const int *settings_host,
                               void *work_dev, int64_t work_bytes, float *motion_out_dev, int *diag_out_dev);
int codetr_track_update4_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                             const float *motion_dev);
int codetr_track_update4_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                              const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                              void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                              int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                              const float *motion_dev);
int codetr_track_update4_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association,
                             const float *motion_dev);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_MOTION_H_ */
