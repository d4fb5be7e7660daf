// The host side of the lens-undistortion stage (include/codetr_undistort.h) as plain C++, no HIP: every check
// codetr_undistort_rgb_u8 makes before it launches, and the per-image table the kernel takes as its argument.  The same
// text is compiled into libcodetr_hip.so and into a stand-alone host program under the sanitizers
// (tests/cabi_c/undistort_host_check.cpp).
#ifndef CODETR_UNDISTORT_ARGS_H_
#define CODETR_UNDISTORT_ARGS_H_

#include <math.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_undistort.h"

namespace undistort {

// rows of `rb` bytes, `rows` of them `pitch` apart from `off`: all inside [0, total)
inline bool rows_inside(int64_t off, int64_t pitch, int64_t rb, int64_t rows, int64_t total) {
  if (off > total || rb > total - off) return false;
  return rows == 1 || pitch <= (total - off - rb) / (rows - 1);
}

inline bool ranges_meet(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

struct Image {
  int64_t src, pitch, dst;
  int model, H, W, Ho, Wo;
  unsigned fill;   // R | G << 8 | B << 16: the dword a pixel is in LDS
  float p[CODETR_UNDISTORT_PARAM_FLOATS];
};
struct ImageTable {  // a kernel argument (3584 bytes of the 4096 a launch may carry), like orient.hip's
  Image f[CODETR_PREPROCESS_BATCH_MAX];
};

// every check of codetr_undistort_rgb_u8 -> 0, `tab` and the largest output sides, or the status to return
inline int check(uintptr_t src, int64_t src_bytes, int64_t N, const int64_t* rows, const float* params, uintptr_t dst,
                 int64_t dst_bytes, ImageTable* tab, int64_t* Hmax, int64_t* Wmax) {
  if (!src || !rows || !params || !dst || !tab || src_bytes <= 0 || dst_bytes <= 0 || N <= 0) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  if (ranges_meet(src, src_bytes, dst, dst_bytes)) return CODETR_E_BADARG;
  *Hmax = 0, *Wmax = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = rows + CODETR_UNDISTORT_ROW_INTS * n;
    const float* p = params + CODETR_UNDISTORT_PARAM_FLOATS * n;
    const int64_t model = r[0], H = r[1], W = r[2], off = r[3], pitch = r[4], Ho = r[5], Wo = r[6], at = r[7], fill = r[8];
    if ((model != CODETR_UNDISTORT_BROWN && model != CODETR_UNDISTORT_FISHEYE) || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
      return CODETR_E_BADARG;
    if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE || Ho > CODETR_FRAME_MAX_SIDE || Wo > CODETR_FRAME_MAX_SIDE)
      return CODETR_E_TOO_LARGE;
    if (off < 0 || pitch < 3 * W || !rows_inside(off, pitch, 3 * W, H, src_bytes)) return CODETR_E_BADARG;
    if (at < 0 || at > dst_bytes || Ho * Wo * 3 > dst_bytes - at) return CODETR_E_BADARG;
    if (fill < 0 || fill > 0xFFFFFF) return CODETR_E_BADARG;
    for (int k = 0; k < CODETR_UNDISTORT_PARAM_FLOATS; ++k)
      if (!isfinite(p[k])) return CODETR_E_BADARG;
    for (int k = 0; k < 8; k += 4) {   // the stored frame's camera, then the rectified image's
      if (!(p[k] > 0.0f) || !(p[k + 1] > 0.0f) || p[k] > CODETR_UNDISTORT_MAX_FOCAL || p[k + 1] > CODETR_UNDISTORT_MAX_FOCAL)
        return CODETR_E_BADARG;
      if (fabsf(p[k + 2]) > CODETR_UNDISTORT_MAX_CENTRE || fabsf(p[k + 3]) > CODETR_UNDISTORT_MAX_CENTRE) return CODETR_E_BADARG;
    }
    for (int64_t m = 0; m < n; ++m) {  // two rectified images may not share a byte
      const int64_t o2 = tab->f[m].dst, e2 = o2 + (int64_t)tab->f[m].Ho * tab->f[m].Wo * 3;
      if (at < e2 && o2 < at + Ho * Wo * 3) return CODETR_E_BADARG;
    }
    Image& im = tab->f[n];
    im.src = off, im.pitch = pitch, im.dst = at;
    im.model = (int)model, im.H = (int)H, im.W = (int)W, im.Ho = (int)Ho, im.Wo = (int)Wo;
    im.fill = (unsigned)((fill >> 16) | (fill & 0xFF00) | ((fill & 0xFF) << 16));
    for (int k = 0; k < CODETR_UNDISTORT_PARAM_FLOATS; ++k) im.p[k] = p[k];
    *Hmax = Ho > *Hmax ? Ho : *Hmax;
    *Wmax = Wo > *Wmax ? Wo : *Wmax;
  }
  return 0;
}

}  // namespace undistort

#endif  // CODETR_UNDISTORT_ARGS_H_
