// The argument checks of include/codetr_draw_tracks.h's entry points, the byte sizes of its state and snapshot, and the
// tables their kernels take: plain host code with no HIP in it, so that a stand-alone program can compile it as well as
// draw_tracks.hip.  Every check runs before any HIP call.
#pragma once
#include <stdint.h>

#include "codetr_draw_tracks.h"

namespace draw_tracks_args {

struct Image {
  int64_t offset;  // bytes, of the image in the buffer
  int H, W;
};
struct Table {  // a kernel argument (512 B), the layout of draw.hip's
  Image img[CODETR_PREPROCESS_BATCH_MAX];
};
struct Rows {  // a kernel argument: the stream of every row, -1 behind the last
  int stream[CODETR_PREPROCESS_BATCH_MAX];
};

inline bool trail_shape_ok(int64_t T, int64_t K) {
  return T >= 1 && T <= CODETR_TRACK_MAX_TRACKS && K >= CODETR_TRAIL_MIN_LENGTH && K <= CODETR_TRAIL_MAX_LENGTH;
}
inline int64_t state_bytes(int64_t T, int64_t K) { return 16 + 16 * T + 4 * T * K; }
inline int64_t snapshot_bytes(int64_t T, int64_t K) { return 16 * T + 4 * T * K; }

// the checks of codetr_trail_update_*; on 0 `rows` is filled
inline int check_update(const void* boxes, const int* count, int64_t N, int64_t Q, const int* stream_of_row, int64_t S,
                        const void* state, int64_t T, int64_t K, const int* ids, int64_t retain, int anchor, int tentative,
                        const void* out, Rows* rows) {
  if (!boxes || !count || !stream_of_row || !state || !ids || !out || N <= 0 || Q <= 0 || S <= 0 || T <= 0 || retain < 1)
    return CODETR_E_BADARG;
  if (K < CODETR_TRAIL_MIN_LENGTH || K > CODETR_TRAIL_MAX_LENGTH) return CODETR_E_BADARG;
  if (anchor != CODETR_TRAIL_CENTER && anchor != CODETR_TRAIL_BOTTOM) return CODETR_E_BADARG;
  if ((tentative != 0 && tentative != 1) || ((uintptr_t)state & 3u) || ((uintptr_t)out & 3u)) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX || Q > CODETR_POSTPROCESS_MAX_Q || T > CODETR_TRACK_MAX_TRACKS || S > 0x7fffffffLL)
    return CODETR_E_TOO_LARGE;
  for (int64_t n = 0; n < CODETR_PREPROCESS_BATCH_MAX; ++n) {
    if (n < N && (stream_of_row[n] < 0 || stream_of_row[n] >= S)) return CODETR_E_BADARG;
    rows->stream[n] = n < N ? stream_of_row[n] : -1;
  }
  return 0;
}

// the checks of codetr_draw_tracks_*: codetr_draw_detections_*'s in their order, then the new operands'; on 0 `tab` is
// filled and *Hmax, *Wmax are the largest sides
inline int check_draw(const void* buf, int64_t buf_bytes, int64_t N, const int64_t* images, const void* boxes,
                      const void* scores, const int64_t* labels, const int* count, int64_t Q, const void* palette,
                      const void* names, int64_t C, int line_width, float alpha, float score_thr, uint32_t text_rgb,
                      int font_scale, int draw_labels, const int* ids, const void* trails, int64_t T, int64_t K,
                      const void* track_palette, int64_t P, int trail_width, float trail_alpha, int color_by, int show_id,
                      int untracked, Table* tab, int64_t* Hmax, int64_t* Wmax) {
  if (!buf || !images || !boxes || !scores || !labels || !count || !palette || !names || buf_bytes <= 0 || N <= 0 ||
      Q <= 0 || C <= 0)
    return CODETR_E_BADARG;
  if (line_width < 1 || line_width > 15 || !(alpha >= 0.f && alpha <= 1.f) || score_thr != score_thr ||
      text_rgb > 0xffffffu || font_scale < 1 || font_scale > 4 || (draw_labels != 0 && draw_labels != 1))
    return CODETR_E_BADARG;
  if (!ids || !track_palette || P <= 0 || trail_width < 1 || trail_width > 15 || !(trail_alpha >= 0.f && trail_alpha <= 1.f))
    return CODETR_E_BADARG;
  if ((color_by != CODETR_COLOR_BY_CLASS && color_by != CODETR_COLOR_BY_TRACK) || (show_id != 0 && show_id != 1) ||
      (untracked != 0 && untracked != 1))
    return CODETR_E_BADARG;
  if (trails && (T <= 0 || K < CODETR_TRAIL_MIN_LENGTH || K > CODETR_TRAIL_MAX_LENGTH || ((uintptr_t)trails & 3u)))
    return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX || Q > CODETR_POSTPROCESS_MAX_Q || C > 65536 || P > 65536 ||
      (trails && T > CODETR_TRACK_MAX_TRACKS))
    return CODETR_E_TOO_LARGE;
  *Hmax = *Wmax = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t off = images[3 * n], H = images[3 * n + 1], W = images[3 * n + 2];
    if (off < 0 || H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_DRAW_MAX_SIDE || W > CODETR_DRAW_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (off > buf_bytes || H * W * 3 > buf_bytes - off) return CODETR_E_BADARG;  // the image must lie in the buffer
    for (int64_t m = 0; m < n; ++m) {  // in place: two images may not share a byte
      const int64_t o2 = tab->img[m].offset, e2 = o2 + (int64_t)tab->img[m].H * tab->img[m].W * 3;
      if (off < e2 && o2 < off + H * W * 3) return CODETR_E_BADARG;
    }
    tab->img[n] = Image{off, (int)H, (int)W};
    *Hmax = H > *Hmax ? H : *Hmax;
    *Wmax = W > *Wmax ? W : *Wmax;
  }
  return 0;
}

}  // namespace draw_tracks_args
