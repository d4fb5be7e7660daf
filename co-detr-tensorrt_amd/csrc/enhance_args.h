// The host side of the contrast-enhancement stage (include/codetr_enhance.h) as plain C++, no HIP: every check
// codetr_enhance_rgb_u8 makes before it launches, the slice and band geometry, and the per-image table the kernels take as
// their argument.  The same text is compiled into libcodetr_hip.so and into a stand-alone host program under the
// sanitizers (tests/cabi_c/enhance_host_check.cpp).
#ifndef CODETR_ENHANCE_ARGS_H_
#define CODETR_ENHANCE_ARGS_H_

#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_enhance.h"

namespace enhance {

// rows of `rb` bytes, `rows` of them `pitch` apart from `off`: all inside [0, total)
inline bool rows_inside(int64_t off, int64_t pitch, int64_t rb, int64_t rows, int64_t total) {
  if (off > total || rb > total - off) return false;
  return rows == 1 || pitch <= (total - off - rb) / (rows - 1);
}

inline bool ranges_meet(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

// whether the spans of two images (first byte of the first row .. last byte of the last) share a byte
inline bool spans_meet(int64_t a, int64_t pa, int64_t ra, int64_t ha, int64_t b, int64_t pb, int64_t rb, int64_t hb) {
  return a < b + (hb - 1) * pb + rb && b < a + (ha - 1) * pa + ra;
}

struct Image {
  int64_t src, spitch, dst, dpitch;
  int H, W, gy, gx, th, tw;
  unsigned T, C, M;   // tile samples, clip count, floor(2^32 / (4 T))
  int S, sr;          // slices per tile, rows per slice
  int br, bands;      // rows per band of a lattice cell, bands per cell
  unsigned base;      // the image's first 1 KB slot of the workspace
};
struct ImageTable {  // a kernel argument (2816 bytes of the 4096 a launch may carry), like undistort.hip's
  Image f[CODETR_PREPROCESS_BATCH_MAX];
};

// steps 1 and "Slices" of the header for one row -> 0 and the geometry in `im`, or the status
inline int geometry(const int64_t* r, Image* im) {
  const int64_t H = r[0], W = r[1], gy = r[6], gx = r[7];
  if (H <= 0 || W <= 0) return CODETR_E_BADARG;
  if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) return CODETR_E_TOO_LARGE;
  if (gy < 1 || gx < 1 || gy > CODETR_ENHANCE_MAX_GRID || gx > CODETR_ENHANCE_MAX_GRID || gy > H || gx > W) return CODETR_E_BADARG;
  const int64_t th = (H + gy - 1) / gy, tw = (W + gx - 1) / gx, T = th * tw;
  if (T > CODETR_ENHANCE_MAX_TILE) return CODETR_E_BADARG;
  int64_t sr = CODETR_ENHANCE_SLICE_PIXELS / tw;
  sr = sr < 1 ? 1 : sr;
  int64_t S = (th + sr - 1) / sr;
  if (S > CODETR_ENHANCE_MAX_SLICES) {
    sr = (th + CODETR_ENHANCE_MAX_SLICES - 1) / CODETR_ENHANCE_MAX_SLICES;
    S = (th + sr - 1) / sr;
  }
  int64_t br = CODETR_ENHANCE_SLICE_PIXELS / tw;  // a lattice cell is at most th x tw
  br = br < 1 ? 1 : br;
  im->H = (int)H, im->W = (int)W, im->gy = (int)gy, im->gx = (int)gx, im->th = (int)th, im->tw = (int)tw;
  im->T = (unsigned)T, im->M = (unsigned)((uint64_t(1) << 32) / (uint64_t)(4 * T));
  im->S = (int)S, im->sr = (int)sr, im->br = (int)br, im->bands = (int)((th + br - 1) / br);
  return 0;
}

// codetr_enhance_workspace_bytes
inline int64_t workspace_bytes(int64_t N, const int64_t* rows) {
  if (!rows || N <= 0) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  int64_t slots = 0;
  for (int64_t n = 0; n < N; ++n) {
    Image im;
    const int rc = geometry(rows + CODETR_ENHANCE_ROW_INTS * n, &im);
    if (rc != 0) return rc;
    slots += (int64_t)im.gy * im.gx * im.S;
  }
  return slots * 1024;   // <= 32 * 32 * 32 * 32 KB = 1 GiB
}

struct Launch {   // grid extents: the largest of each over the images
  int slices, tiles, bands, cells;
};

// every check of codetr_enhance_rgb_u8 -> 0, `tab` and the grids, or the status to return
inline int check(uintptr_t src, int64_t src_bytes, int64_t N, const int64_t* rows, uintptr_t dst, int64_t dst_bytes, uintptr_t ws,
                 int64_t ws_bytes, ImageTable* tab, Launch* grid) {
  if (!src || !rows || !dst || !ws || !tab || !grid || src_bytes <= 0 || dst_bytes <= 0 || ws_bytes <= 0 || N <= 0) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  const bool in_place = src == dst;
  if (in_place ? src_bytes != dst_bytes : ranges_meet(src, src_bytes, dst, dst_bytes)) return CODETR_E_BADARG;
  if ((ws & 3u) || ranges_meet(ws, ws_bytes, src, src_bytes) || ranges_meet(ws, ws_bytes, dst, dst_bytes)) return CODETR_E_BADARG;
  *grid = Launch{0, 0, 0, 0};
  int64_t slots = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = rows + CODETR_ENHANCE_ROW_INTS * n;
    Image& im = tab->f[n];
    const int rc = geometry(r, &im);
    if (rc != 0) return rc;
    const int64_t H = r[0], W = r[1], off = r[2], pitch = r[3], at = r[4], dpitch = r[5], C = r[8];
    if (C < 1 || C > (int64_t)im.T) return CODETR_E_BADARG;
    if (off < 0 || pitch < 3 * W || !rows_inside(off, pitch, 3 * W, H, src_bytes)) return CODETR_E_BADARG;
    if (at < 0 || dpitch < 3 * W || !rows_inside(at, dpitch, 3 * W, H, dst_bytes)) return CODETR_E_BADARG;
    if (in_place && (at != off || dpitch != pitch)) return CODETR_E_BADARG;
    for (int64_t m = 0; m < n; ++m) {  // two enhanced images may not share a byte
      const Image& o = tab->f[m];
      if (spans_meet(at, dpitch, 3 * W, H, o.dst, o.dpitch, 3 * (int64_t)o.W, o.H)) return CODETR_E_BADARG;
    }
    im.src = off, im.spitch = pitch, im.dst = at, im.dpitch = dpitch, im.C = (unsigned)C;
    im.base = (unsigned)slots;
    slots += (int64_t)im.gy * im.gx * im.S;
    const int tiles = im.gy * im.gx, cells = (im.gy + 1) * (im.gx + 1);
    grid->slices = im.S > grid->slices ? im.S : grid->slices;
    grid->tiles = tiles > grid->tiles ? tiles : grid->tiles;
    grid->bands = im.bands > grid->bands ? im.bands : grid->bands;
    grid->cells = cells > grid->cells ? cells : grid->cells;
  }
  if (slots * 1024 > ws_bytes) return CODETR_E_BADARG;
  return 0;
}

}  // namespace enhance

#endif  // CODETR_ENHANCE_ARGS_H_
