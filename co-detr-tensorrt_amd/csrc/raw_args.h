// The host side of the raw Bayer stage (include/codetr_raw.h) as plain C++, no HIP: the multipliers of the rule's step 1,
// every check codetr_raw_to_rgb_u8 makes before it launches, and the border fold of step 2 -- the one function the kernel
// shares, so it is __host__ __device__ under hipcc.  The same text is compiled into libcodetr_hip.so and into a
// stand-alone host program under the sanitizers (tests/cabi_c/raw_args_host_check.cpp).
#ifndef CODETR_RAW_ARGS_H_
#define CODETR_RAW_ARGS_H_

#include <math.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_raw.h"

#ifdef __HIPCC__
#define RAW_HD __host__ __device__ __forceinline__
#else
#define RAW_HD inline
#endif

namespace raw {

// step 2: index i on an axis of length n >= 1 -> the sample it reads, in [0, n)
RAW_HD int fold(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

// step 1: the three multipliers; false for settings the rule does not take
inline bool multipliers(int64_t black, int64_t white, const double* gains, int64_t* m) {
  if (black < 0 || white > 65535 || white <= black) return false;
  for (int c = 0; c < 3; ++c) {
    const double g = gains[c];
    if (!(g >= 0.0) || !isfinite(g)) return false;
    const double v = floor(g * 4294901760.0 / (double)(white - black) + 0.5);
    if (!(v < 4294967296.0)) return false;
    m[c] = (int64_t)v;
  }
  return true;
}

// rows of `rb` bytes, `rows` of them `pitch` apart from `off`: all inside [0, total)
inline bool rows_inside(int64_t off, int64_t pitch, int64_t rb, int64_t rows, int64_t total) {
  if (off > total || rb > total - off) return false;
  return rows == 1 || pitch <= (total - off - rb) / (rows - 1);
}

inline bool ranges_meet(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

struct Frame {
  int64_t src, pitch, dst;
  int ry, rx, H, W;
};
struct Checked {
  Frame f[CODETR_PREPROCESS_BATCH_MAX];
  int bytes;            // per sample: 1 or 2
  int method;
  unsigned black, white, m[3];
  int64_t Hmax, Wmax;
};

// every check of codetr_raw_to_rgb_u8 -> 0 and `out`, or the status to return
inline int check(uintptr_t src, int64_t src_bytes, int64_t N, const int64_t* rows, const int64_t* settings, uintptr_t lut,
                 uintptr_t dst, int64_t dst_bytes, Checked* out) {
  if (!src || !rows || !settings || !lut || !dst || src_bytes <= 0 || dst_bytes <= 0 || N <= 0) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  if (lut & 15u) return CODETR_E_BADARG;
  if (ranges_meet(src, src_bytes, dst, dst_bytes) || ranges_meet(lut, CODETR_RAW_LUT_BYTES, dst, dst_bytes)) return CODETR_E_BADARG;
  const int64_t method = settings[0], black = settings[1], white = settings[2];
  if (method != CODETR_RAW_MALVAR && method != CODETR_RAW_BILINEAR) return CODETR_E_BADARG;
  if (black < 0 || white > 65535 || white <= black) return CODETR_E_BADARG;
  for (int c = 0; c < 3; ++c) {
    if (settings[3 + c] < 0 || settings[3 + c] > 0xFFFFFFFFll) return CODETR_E_BADARG;
    out->m[c] = (unsigned)settings[3 + c];
  }
  out->method = (int)method, out->black = (unsigned)black, out->white = (unsigned)white;
  out->bytes = 0, out->Hmax = 0, out->Wmax = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = rows + CODETR_RAW_ROW_INTS * n;
    const int64_t pattern = r[0], bits = r[1], H = r[2], W = r[3], off = r[4], pitch = r[5], at = r[6];
    if (pattern < CODETR_RAW_RGGB || pattern > CODETR_RAW_BGGR || bits < 8 || bits > 16 || H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) return CODETR_E_TOO_LARGE;
    const int bytes = bits == 8 ? 1 : 2;
    if (out->bytes && out->bytes != bytes) return CODETR_E_BADARG;
    out->bytes = bytes;
    if (white > (1ll << bits) - 1) return CODETR_E_BADARG;
    if (off < 0 || pitch < bytes * W || !rows_inside(off, pitch, bytes * W, H, src_bytes)) return CODETR_E_BADARG;
    if (bytes == 2 && (((src + (uintptr_t)off) | (uintptr_t)pitch) & 1u)) return CODETR_E_BADARG;
    if (at < 0 || at > dst_bytes || H * W * 3 > dst_bytes - at) return CODETR_E_BADARG;
    for (int64_t k = 0; k < n; ++k) {  // two images may not share a byte
      const int64_t o2 = out->f[k].dst, e2 = o2 + (int64_t)out->f[k].H * out->f[k].W * 3;
      if (at < e2 && o2 < at + H * W * 3) return CODETR_E_BADARG;
    }
    out->f[n] = Frame{off, pitch, at, (int)(pattern >> 1), (int)(pattern & 1), (int)H, (int)W};
    out->Hmax = H > out->Hmax ? H : out->Hmax;
    out->Wmax = W > out->Wmax ? W : out->Wmax;
  }
  return 0;
}

}  // namespace raw

#endif  // CODETR_RAW_ARGS_H_
