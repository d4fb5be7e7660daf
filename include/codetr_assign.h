/* codetr_assign.h -- companion header of codetr_hip.h: linear assignment on the GPU (one workgroup per problem) and the
 * tracker with an optimal association next to the greedy one.  Exported from the same libcodetr_hip.so; versioned on its
 * own (a self-contained addition does not touch CODETR_HIP_ABI_VERSION).  Error codes and the limits
 * CODETR_PREPROCESS_BATCH_MAX / CODETR_POSTPROCESS_MAX_Q / CODETR_TRACK_MAX_TRACKS are codetr_hip.h's.
 *
 * Beyond the reference (its Inferencer has no tracker and its training path is not part of this library).  mmdet's
 * ByteTracker solves an assignment problem per association (`lap.lapjv`); codetr_hip.h's "Tracking" picks greedily and
 * says so.  This header adds the assignment form.  The rule below is stated in integer arithmetic only, so that a
 * restatement (tests/assign_ref.py, tests/track_assign_ref.py) reproduces every match, not just the optimum's value.
 *
 * The problem: n rows, m columns, integer gains g[i][j] in [0, CODETR_ASSIGN_MAX_GAIN].  A matching gives every row at
 *   most one column and every column at most one row; the result maximises the sum of the gains of its pairs.  A pair of
 *   gain 0 is never reported: its row is unmatched (-1).  Nothing is decided by a floating-point comparison of sums.
 * One result, not "any optimum": the matching this procedure yields (shortest augmenting paths, Jonker-Volgenant /
 *   Hungarian form, over the costs c[i][j] = -g[i][j]).  All quantities are 64-bit integers.
 *   Columns: M = max(n, m); the columns m .. M - 1 are virtual and have gain 0 for every row, so there is a column for
 *   every row.  Duals u[n] and v[M] start at 0; owner[j] = -1 (column j is free) for every j.
 *   For the rows i = 0, 1, .. n - 1 in this order, one augmentation:
 *     dist[j] = INF and visited[j] = 0 for every column; the current row r = i, its distance D = 0, pred of what it
 *     reaches = -1 (the start).  Repeat, at most M + 1 times:
 *       relax: for every column j not visited, d = D + c[r][j] - u[r] - v[j]; if d < dist[j]: dist[j] = d, pred[j] = the
 *         column through which r was reached (-1 for r = i);
 *       pick: j* = the column not visited of the least dist, ties to the lowest column index; D = dist[j*];
 *         visited[j*] = 1; if owner[j*] = -1 the search ends with the sink j*, otherwise r = owner[j*] and the next
 *         round relaxes from it (reached through j*).
 *     dual update, once per augmentation, with the final D: for every visited column j: v[j] -= D - dist[j], and
 *       u[owner[j]] += D - dist[j] where j has an owner; u[i] += D.  (The same duals as an update by the step's delta
 *       after every pick: there a visited column collects every later delta, D - dist[j] in all.)
 *     augment: from the sink back along pred: owner[j] = owner[pred[j]], and owner[j] = i where pred[j] = -1.
 *   Result: match[owner[j]] = j for every real column j < m with an owner and g[owner[j]][j] > 0; every other row -1;
 *   total = the sum of the gains of those pairs.
 *   Bounds: a search visits one more column per round and a free column always exists (fewer than M rows are matched),
 *   so it ends within M rounds; the loops are counted (M + 1 rounds, n augmentations, M + 1 steps back along pred): a
 *   defect ends in a wrong answer, never in a spinning workgroup.  |u|, |v| stay below n * CODETR_ASSIGN_MAX_GAIN in
 *   every case tried (1.0e9 at 512 x 1024); they are 64-bit, dist likewise.
 *
 * codetr_assign_i32: B problems of one shape in one launch, one workgroup of 256 threads per problem (csrc/assign.hip).
 *     gain_dev       [B, n, m] int32; every value is clamped into [0, CODETR_ASSIGN_MAX_GAIN] as it is read
 *     match_out_dev  [B, n] int32: the column of every row, -1 for unmatched
 *     total_out_dev  [B] int64: the sum of the (clamped) gains of the matched pairs
 *   A thread owns the columns tid, tid + 256, ..: dist and visited live in its registers, u, v, pred and owner in LDS
 *   (8 n + 12 M + 96 bytes, 16.1 KB at the limits).  A round is one relax of the thread's columns, one workgroup arg-min
 *   (wave shuffles, double-buffered partials) and one barrier.
 *   CODETR_E_BADARG for a null pointer or B, n or m <= 0; CODETR_E_TOO_LARGE for n > CODETR_ASSIGN_MAX_ROWS,
 *   m > CODETR_ASSIGN_MAX_COLS or B > 65535.  All checks run before any HIP call.
 *
 * codetr_track_update2_{f16,bf16,f32}: codetr_track_update_* (codetr_hip.h, "Tracking") with one more argument:
 *     association  CODETR_ASSOCIATION_GREEDY: the rule of codetr_hip.h as it is -- the same ids, the same state bytes as
 *                  codetr_track_update_*.  CODETR_ASSOCIATION_OPTIMAL: steps 3 to 5 become assignment problems.
 *   The state layout and codetr_track_state_bytes are unchanged: a stream may switch association between calls.
 *   Steps 1, 2 and 6 to 9 are unchanged.  The three phases keep their track sets, candidate classes, values and thresholds
 *   (A: confirmed tracks x high candidates, threshold match high; B: tentative tracks x the high candidates still free,
 *   match tentative; C: confirmed tracks still unmatched with last == f - 1 x low candidates, plain iou, match low).  In a
 *   phase with threshold thr:
 *     a pair (track, candidate) is eligible exactly as today: equal labels, the candidate free and of the phase's class,
 *       value >= thr (a NaN compares false);
 *     its gain: g = 1 + (int)(fminf(value - thr, 2.0f) * 1048576.0f) -- one fp32 subtraction, a clamp, an exact
 *       multiplication by 2^20, truncation -- in 1 .. CODETR_ASSIGN_MAX_GAIN; a pair that is not eligible has gain 0;
 *     rows: the phase's tracks with at least one eligible pair, in ascending slot order; columns: ALL candidate rows
 *       j = 0 .. cnt - 1 of the frame (those of another class, taken, or taking no part have gain 0 for every row);
 *       virtual columns as above when there are more rows than candidates;
 *     the procedure above; a row that ends on a pair of gain 0 stays unmatched in this phase; a matched candidate is no
 *       longer free for the later phases.
 *   The objective corresponds to mmdet's lapjv(1 - value, extend_cost=True, cost_limit=1 - thr), which minimises the sum
 *   of (cost - cost_limit) over the matched pairs, i.e. maximises the sum of (value - thr) -- mmdet as recalled: parity
 *   stays unpinned.  This library's own deviations: the + 1, which makes every eligible pair worth taking when nothing
 *   competes (a pair with value == thr counts), the 2^-20 step of the gains, the stated tie rule, and the label comparison
 *   and values of codetr_hip.h.
 *   The gains are computed on the fly from the boxes in LDS; there is no T x Q matrix.  LDS: the tracker's
 *   (codetr_hip.h) + 8 T + 12 max(T, Q) + 96 bytes, 114 KB at T = 512, Q = 1024.
 *   Errors: those of codetr_track_update_*, and CODETR_E_BADARG for an association that is neither of the two.
 */
#ifndef CODETR_ASSIGN_H_
#define CODETR_ASSIGN_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_ASSIGN_ABI_VERSION 1
#define CODETR_ASSIGN_MAX_ROWS 512
#define CODETR_ASSIGN_MAX_COLS 1024
#define CODETR_ASSIGN_MAX_GAIN 2097153
#define CODETR_ASSOCIATION_GREEDY 0
#define CODETR_ASSOCIATION_OPTIMAL 1

int codetr_assign_abi_version(void);
int codetr_assign_i32(void *stream, const int *gain_dev, int64_t B, int64_t n, int64_t m, int *match_out_dev,
                      int64_t *total_out_dev);
int codetr_track_update2_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association);
int codetr_track_update2_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                              const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                              void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                              int64_t tentatives, int weight_iou, int *track_id_out_dev, int association);
int codetr_track_update2_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev, int association);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_ASSIGN_H_ */
