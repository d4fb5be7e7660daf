/* codetr_draw_tracks.h -- companion header of codetr_hip.h: the tracker's output on the picture.  One colour per identity,
 * the id in the label, and a trail of where the object has been, drawn in place in the packed RGB images the
 * pre-processing kernels read.  Exported from the same libcodetr_hip.so; versioned on its own (CODETR_HIP_ABI_VERSION and
 * the other companion headers are as they were).  Error codes and the limits CODETR_PREPROCESS_BATCH_MAX /
 * CODETR_POSTPROCESS_MAX_Q / CODETR_TRACK_MAX_TRACKS / CODETR_DRAW_MAX_SIDE are codetr_hip.h's.
 *
 * Beyond the reference (its Inferencer neither tracks nor draws tracks).  The three things are those of mmdet's
 * TrackLocalVisualizer (a colour per id, the id in the label) and of supervision's TraceAnnotator (the trail); the
 * rendering is this library's own and parity with either is unpinned (neither is installed where this is tested).
 * Limits: a trail is an integer polyline of capsules, not antialiased; its alpha is constant, it does not fade; its points
 * are image positions as they were seen -- a camera motion the tracker compensates (codetr_motion.h) does not move them.
 *
 * The rule is exact: integers, apart from the fp32 steps of codetr_hip.h's drawing rule ("Visualisation": pixel_coord,
 * the score's tenths, A of an alpha), so that a restatement (tests/draw_tracks_ref.py) reproduces every byte.
 *     pixel_coord(v) = (int)floorf(fminf(fmaxf(v, -16384.0f), 16383.0f) + 0.5f)   (one fp32 rounding in the sum)
 *     blend(p, c, A) = (p * (256 - A) + c * A + 128) >> 8 per channel
 *
 * ---- Trail state: one per stream, T = max_tracks entries (1..CODETR_TRACK_MAX_TRACKS), K = length points (2..64) ----
 *   codetr_trail_state_bytes(T, K) = 16 + 16 T + 4 T K bytes, little endian, 4-byte aligned.  A zero-filled state is a
 *   fresh stream.
 *     int32 f, 0, 0, 0          the header: f counts the stream's frames (it wraps after 2^31 of them)
 *     int32 id[T]               0 = a free entry, and then every other field of the entry, its ring included, is 0
 *     int32 last[T]             the frame f of the entry's newest point
 *     int32 len[T]              points held, 1..K
 *     int32 head[T]             the ring slot of the OLDEST point
 *     (int16 x, int16 y) ring[T][K]
 *   Snapshot of one row: codetr_trail_snapshot_bytes(T, K) = 16 T + 4 T K bytes, what the drawing reads.
 *     int32 id[T], int32 len[T]           the entry's, after the row's update
 *     (int16 x0, y0, x1, y1) box[T]        the inclusive bounding box of the entry's len points (zeros for a free entry)
 *     (int16 x, int16 y) points[T][K]      the len points OLDEST FIRST, zeros behind them
 *
 * codetr_trail_update_{f16,bf16,f32}: the operands of codetr_track_update_* -- boxes_dev [N, Q, 4], scores_dev and
 *   labels_dev [N, Q] (not read by this version; may be NULL), count_dev [N], N <= CODETR_PREPROCESS_BATCH_MAX rows of
 *   Q <= CODETR_POSTPROCESS_MAX_Q, stream_of_row_host [N] in [0, S), state_dev [S] states -- and
 *     track_ids_dev [N, Q] int32   as codetr_track_update*_ wrote it: negative while the track is tentative, 0 = no track
 *     retain >= 1                  an entry without a point for `retain` frames is freed
 *     anchor                       CODETR_TRAIL_CENTER: the box centre; CODETR_TRAIL_BOTTOM: the middle of its lower edge
 *     tentative                    0: rows with id > 0 take part; 1: rows with id != 0
 *     trails_out_dev               [N] snapshots, every byte written
 *   One workgroup per stream walks the stream's rows in row order (csrc/draw_tracks.hip, trail_update_kernel), the state in
 *   LDS; it is read and written back once, a stream without a row is not touched.  Per row n of a stream:
 *     1. every entry with id != 0 and f - last >= retain is zeroed (its ring too);
 *     2. candidates are the rows j < clamp(count[n], 0, Q) with track_ids[n, j] > 0 (!= 0 with `tentative`; never
 *        INT32_MIN) whose four coordinates, widened to fp32 exactly, are finite.  key = |id|.  The row's point is
 *            (pixel_coord((x1 + x2) * 0.5f), pixel_coord(ya)),  ya = (y1 + y2) * 0.5f (CENTER) or y2 (BOTTOM):
 *        the sum is rounded once, the product once, nothing is contracted.  Of several candidates with one key only the
 *        one with the lowest j counts;
 *     3. a candidate whose key is the id of an entry appends to it: if len < K the point goes to slot (head + len) % K and
 *        len += 1, otherwise it overwrites slot head and head = (head + 1) % K; last = f;
 *     4. the remaining candidates, j ascending, take the free entries, index ascending (those freed in step 1 included):
 *        id = key, last = f, len = 1, head = 0, slot 0 = the point.  Without a free entry the candidate is dropped;
 *     5. the row's snapshot is written;
 *     6. f += 1.
 *   CODETR_E_BADARG for a null pointer (boxes, count, streams, states, ids, snapshots), N, Q, S, max_tracks <= 0, length
 *   outside 2..64, a stream index outside [0, S), retain < 1, an anchor or `tentative` outside its set, a state or a
 *   snapshot pointer that is not 4-byte aligned; CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX,
 *   Q > CODETR_POSTPROCESS_MAX_Q, max_tracks > CODETR_TRACK_MAX_TRACKS.  All checks run before any HIP call.
 *
 * codetr_draw_tracks_{f16,bf16,f32}: the operands and checks of codetr_draw_detections_* with
 *   Q <= CODETR_POSTPROCESS_MAX_Q, and
 *     track_ids_dev [N, Q] int32          the id of every detection row
 *     trails_dev, max_tracks, length      [N] snapshots of codetr_trail_update_*, image n's at n * snapshot bytes; NULL
 *                                         (then T and K are ignored): no trails
 *     track_palette_dev [P, 3] uint8      the colour of identity i is track_palette[(i - 1) % P], P in 1..65536
 *     trail_width w in 1..15;  trail_alpha in [0, 1],  At = (int)(trail_alpha * 256.0f + 0.5f)
 *     color_by                            CODETR_COLOR_BY_CLASS / CODETR_COLOR_BY_TRACK
 *     show_id, untracked                  0 / 1
 *   Per image, in this order:
 *   Layer 0, trails: the snapshot's entries with id != 0 and len >= 1, entry index ascending, in the colour of id.  A
 *     trail covers the union of the capsules of its len - 1 segments (points i -> i + 1); a trail of one point is a disc
 *     (the segment P0 -> P0).  EVERY COVERED PIXEL IS BLENDED ONCE PER TRAIL, blend(p, colour, At), however many of its
 *     segments cover it.  Pixel (x, y) is covered by segment P0 -> P1 iff, with d = P1 - P0, e = (x, y) - P0, L = d.d,
 *     t = e.d, all in int64:
 *         L == 0 or t <= 0:   e.e <= (w * w) / 4                                   (integer division)
 *         t >= L:             g.g <= (w * w) / 4,  g = (x, y) - P1
 *         otherwise:          cross * cross <= (w * w * L) / 4,  cross = e.x * d.y - e.y * d.x.
 *     Bound: coordinates lie in [-16384, 16383] and pixels in [0, 16383], so |d|, |e| <= 32767 per component,
 *     L <= 2^31, |cross| < 2^31 and cross^2 < 2^62; w * w * L < 2^39: nothing overflows int64.
 *   Layer 1, box edges, as codetr_hip.h's, for the drawn rows j ascending, with id = track_ids[n, j]: a row with id == 0
 *     is drawn as there when `untracked` is 1 and not at all (no edge, no label) when it is 0; the colour of a row is
 *     track_palette[(|id| - 1) % P] when color_by is TRACK and id != 0, palette[label] otherwise.
 *   Layer 2, labels, as codetr_hip.h's; with show_id and id != 0 the text is "#<|id|> <name>: <percent>", '~' in place of
 *     '#' while id < 0; |id| in decimal without leading zeros (up to 10 digits: |INT32_MIN| = 2147483648).  The grid's
 *     width follows the text's length; everything else (origin, scale, font, patch) is unchanged.
 *   Everything is clipped to the image.  A pixel that no layer touches is never written and a byte outside the images
 *   never is.  With every id 0, untracked = 1 and trails_dev NULL the result is codetr_draw_detections_*'s, byte for byte.
 *   One 256-thread workgroup per 64 x 16 tile (csrc/draw_tracks.hip, draw_tracks_kernel); no workspace.  Beyond
 *   codetr_draw_detections_*'s codes: CODETR_E_BADARG for a null track_ids_dev or track_palette_dev, P <= 0, trail_width
 *   outside 1..15, trail_alpha outside [0, 1], color_by, show_id or untracked outside their sets, and -- with trails_dev
 *   -- max_tracks <= 0, length outside 2..64 or a pointer that is not 4-byte aligned; CODETR_E_TOO_LARGE for
 *   Q > CODETR_POSTPROCESS_MAX_Q, P > 65536, max_tracks > CODETR_TRACK_MAX_TRACKS.  All checks run before any HIP call.
 */
#ifndef CODETR_DRAW_TRACKS_H_
#define CODETR_DRAW_TRACKS_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_DRAW_TRACKS_ABI_VERSION 1
#define CODETR_TRAIL_MIN_LENGTH 2
#define CODETR_TRAIL_MAX_LENGTH 64
#define CODETR_TRAIL_CENTER 0
#define CODETR_TRAIL_BOTTOM 1
#define CODETR_COLOR_BY_CLASS 0
#define CODETR_COLOR_BY_TRACK 1

int codetr_draw_tracks_abi_version(void);
int64_t codetr_trail_state_bytes(int64_t max_tracks, int64_t length);
int64_t codetr_trail_snapshot_bytes(int64_t max_tracks, int64_t length);
int codetr_trail_update_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                            const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                            void *state_dev, int64_t max_tracks, int64_t length, const int *track_ids_dev,
                            int64_t retain, int anchor, int tentative, void *trails_out_dev);
int codetr_trail_update_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, int64_t length, const int *track_ids_dev,
                             int64_t retain, int anchor, int tentative, void *trails_out_dev);
int codetr_trail_update_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                            const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                            void *state_dev, int64_t max_tracks, int64_t length, const int *track_ids_dev,
                            int64_t retain, int anchor, int tentative, void *trails_out_dev);
int codetr_draw_tracks_f16(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                           const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                           const int *count_dev, int64_t Q, const unsigned char *palette_dev,
                           const unsigned char *names_dev, int64_t C, int line_width, float alpha, float score_thr,
                           uint32_t text_rgb, int font_scale, int draw_labels, const int *track_ids_dev,
                           const void *trails_dev, int64_t max_tracks, int64_t length,
                           const unsigned char *track_palette_dev, int64_t P, int trail_width, float trail_alpha,
                           int color_by, int show_id, int untracked);
int codetr_draw_tracks_bf16(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                            const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                            const int *count_dev, int64_t Q, const unsigned char *palette_dev,
                            const unsigned char *names_dev, int64_t C, int line_width, float alpha, float score_thr,
                            uint32_t text_rgb, int font_scale, int draw_labels, const int *track_ids_dev,
                            const void *trails_dev, int64_t max_tracks, int64_t length,
                            const unsigned char *track_palette_dev, int64_t P, int trail_width, float trail_alpha,
                            int color_by, int show_id, int untracked);
int codetr_draw_tracks_f32(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                           const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                           const int *count_dev, int64_t Q, const unsigned char *palette_dev,
                           const unsigned char *names_dev, int64_t C, int line_width, float alpha, float score_thr,
                           uint32_t text_rgb, int font_scale, int draw_labels, const int *track_ids_dev,
                           const void *trails_dev, int64_t max_tracks, int64_t length,
                           const unsigned char *track_palette_dev, int64_t P, int trail_width, float trail_alpha,
                           int color_by, int show_id, int untracked);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_DRAW_TRACKS_H_ */
