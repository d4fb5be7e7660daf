// The argument checks of include/codetr_redact.h's entry points and the image table their kernel takes: plain host code
// with no HIP in it, so that a stand-alone program can compile it (tests/cabi_c/redact_host_check.cpp) as well as
// redact.hip.  Every check runs before any HIP call.
#pragma once
#include <stdint.h>

#include "codetr_redact.h"

namespace redact_args {

struct Image {
  int64_t offset;  // bytes, of the image in the buffer
  int64_t work;    // cells, of the image's means in the workspace (BLUR)
  int H, W;
};
struct Table {  // a kernel argument (768 B)
  Image img[CODETR_PREPROCESS_BATCH_MAX];
};

inline int log2_cell(int64_t cell) {  // 2..6, or -1 for a cell outside {4, 8, 16, 32, 64}
  for (int s = 2; s <= 6; ++s)
    if (cell == ((int64_t)1 << s)) return s;
  return -1;
}

// N and the rows' H and W (not the offsets): -> the cells of all images, or a negative code; tab may be null
inline int64_t count_cells(int64_t N, const int64_t* images, int64_t cell, Table* tab) {
  if (!images || N <= 0 || log2_cell(cell) < 0) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  int64_t cells = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t H = images[3 * n + 1], W = images[3 * n + 2];
    if (H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_DRAW_MAX_SIDE || W > CODETR_DRAW_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (tab) tab->img[n].work = cells, tab->img[n].H = (int)H, tab->img[n].W = (int)W;
    cells += ((H + cell - 1) / cell) * ((W + cell - 1) / cell);
  }
  return cells;
}

// the checks of codetr_redact_detections_*; on 0 `tab` is filled and *Hmax, *Wmax are the largest sides
inline int check(const void* buf, int64_t buf_bytes, int64_t N, const int64_t* images, const void* boxes, const void* scores,
                 const int64_t* labels, const int* count, int64_t Q, const unsigned char* select, int64_t C, int mode,
                 int shape, int cell, float score_thr, float expand, uint32_t fill_rgb, const void* work, int64_t work_bytes,
                 Table* tab, int64_t* Hmax, int64_t* Wmax) {
  if (!buf || !images || !boxes || !scores || !labels || !count || buf_bytes <= 0 || N <= 0 || Q <= 0) return CODETR_E_BADARG;
  if (select && C <= 0) return CODETR_E_BADARG;
  if (mode != CODETR_REDACT_PIXELATE && mode != CODETR_REDACT_BLUR && mode != CODETR_REDACT_FILL) return CODETR_E_BADARG;
  if (shape != CODETR_REDACT_BOX && shape != CODETR_REDACT_ELLIPSE) return CODETR_E_BADARG;
  if (log2_cell(cell) < 0 || score_thr != score_thr || !(expand >= 0.f && expand <= 1.f) || fill_rgb > 0xffffffu)
    return CODETR_E_BADARG;
  if (Q > CODETR_DRAW_MAX_Q || (select && C > 65536)) return CODETR_E_TOO_LARGE;
  const int64_t cells = count_cells(N, images, cell, tab);
  if (cells < 0) return (int)cells;
  *Hmax = *Wmax = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t off = images[3 * n], H = images[3 * n + 1], W = images[3 * n + 2];
    if (off < 0 || off > buf_bytes || H * W * 3 > buf_bytes - off) return CODETR_E_BADARG;  // the image lies in the buffer
    for (int64_t m = 0; m < n; ++m) {  // in place: two images may not share a byte
      const int64_t o2 = tab->img[m].offset, e2 = o2 + (int64_t)tab->img[m].H * tab->img[m].W * 3;
      if (off < e2 && o2 < off + H * W * 3) return CODETR_E_BADARG;
    }
    tab->img[n].offset = off;
    *Hmax = H > *Hmax ? H : *Hmax;
    *Wmax = W > *Wmax ? W : *Wmax;
  }
  if (mode == CODETR_REDACT_BLUR && (!work || ((uintptr_t)work & 3u) || work_bytes < 4 * cells)) return CODETR_E_BADARG;
  return 0;
}

}  // namespace redact_args
