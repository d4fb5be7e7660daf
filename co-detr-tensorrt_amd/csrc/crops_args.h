// The argument checks of include/codetr_crops.h's entry points, the image table their kernels take and the integer
// rules both sides of the launch share (the inner rectangle of a fit, the taps of an output sample): plain host code with
// no HIP in it, so that a stand-alone program can compile it (tests/cabi_c/crops_host_check.cpp) as well as crops.hip.
// Every check runs before any HIP call.
#pragma once
#include <stdint.h>

#include "codetr_crops.h"

#if defined(__HIPCC__)
#define CROPS_HD __host__ __device__ inline
#else
#define CROPS_HD inline
#endif

namespace crops_args {

struct Image {
  int64_t offset;  // bytes, of the image in the buffer
  int H, W;
};
struct Table {  // a kernel argument (512 B)
  Image img[CODETR_PREPROCESS_BATCH_MAX];
};

// the inner rectangle (ox, oy, iw, ih) of an Rw x Rh region in a w x h output
CROPS_HD void inner_rect(int fit, int Rw, int Rh, int w, int h, int* ox, int* oy, int* iw, int* ih) {
  *iw = w, *ih = h;
  if (fit == CODETR_CROPS_PAD) {
    if (Rw * h >= Rh * w) {
      const int v = (2 * Rh * w + Rw) / (2 * Rw);
      *ih = v < 1 ? 1 : v > h ? h : v;
    } else {
      const int v = (2 * Rw * h + Rh) / (2 * Rh);
      *iw = v < 1 ? 1 : v > w ? w : v;
    }
  }
  *ox = (w - *iw) / 2, *oy = (h - *ih) / 2;
}

// weight of source pixel s for output sample j along an axis (region length R, inner length n), units of 1 / (2n) pixel
CROPS_HD int tap_weight(int j, int s, int n, int R) {
  const int S = 2 * (n > R ? n : R);
  int d = (2 * s + 1) * n - (2 * j + 1) * R;
  d = d < 0 ? -d : d;
  return d < S ? S - d : 0;
}
// [lo, hi] holds every source pixel with a positive weight for output sample j (its ends may have weight 0)
CROPS_HD void tap_range(int j, int n, int R, int* lo, int* hi) {
  const int S = 2 * (n > R ? n : R), c = (2 * j + 1) * R;
  const int a = c - S < 0 ? 0 : (c - S) / (2 * n), b = (c + S) / (2 * n);
  *lo = a, *hi = b > R - 1 ? R - 1 : b;
}

// the checks of codetr_crop_detections_*; on 0 `tab` is filled and *Wmax is the largest width
inline int check(const void* buf, int64_t buf_bytes, int64_t N, const int64_t* images, const void* boxes, const void* scores,
                 const int64_t* labels, const int* count, int64_t Q, const unsigned char* select, int64_t C, int out_w,
                 int out_h, int max_per_img, int fit, float score_thr, float expand, uint32_t pad_rgb, const void* crops,
                 const int* counts, const int* table, const void* tensor, int tensor_type, const float* mean,
                 const float* stdv, Table* tab, int64_t* Wmax) {
  if (!buf || !images || !boxes || !scores || !labels || !count || !crops || !counts || !table || buf_bytes <= 0 || N <= 0 ||
      Q <= 0)
    return CODETR_E_BADARG;
  if (select && C <= 0) return CODETR_E_BADARG;
  if (out_w < CODETR_CROPS_MIN_SIDE || out_h < CODETR_CROPS_MIN_SIDE || max_per_img < 1) return CODETR_E_BADARG;
  if (fit != CODETR_CROPS_STRETCH && fit != CODETR_CROPS_PAD) return CODETR_E_BADARG;
  if (score_thr != score_thr || !(expand >= 0.f && expand <= 1.f) || pad_rgb > 0xffffffu) return CODETR_E_BADARG;
  if ((uintptr_t)table & 3u) return CODETR_E_BADARG;
  if (tensor_type < CODETR_CROPS_TENSOR_NONE || tensor_type > CODETR_CROPS_TENSOR_BF16) return CODETR_E_BADARG;
  if (tensor_type != CODETR_CROPS_TENSOR_NONE) {
    if (!tensor || !mean || !stdv) return CODETR_E_BADARG;
    if ((uintptr_t)tensor & (tensor_type == CODETR_CROPS_TENSOR_F32 ? 3u : 1u)) return CODETR_E_BADARG;  // its element's size
    for (int c = 0; c < 3; ++c)
      if (mean[c] != mean[c] || stdv[c] != stdv[c] || stdv[c] == 0.f) return CODETR_E_BADARG;
  }
  if (N > CODETR_PREPROCESS_BATCH_MAX || Q > CODETR_DRAW_MAX_Q || (select && C > 65536)) return CODETR_E_TOO_LARGE;
  if (out_w > CODETR_CROPS_MAX_SIDE || out_h > CODETR_CROPS_MAX_SIDE || max_per_img > CODETR_CROPS_MAX_PER_IMG)
    return CODETR_E_TOO_LARGE;
  *Wmax = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t off = images[3 * n], H = images[3 * n + 1], W = images[3 * n + 2];
    if (H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_DRAW_MAX_SIDE || W > CODETR_DRAW_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (off < 0 || off > buf_bytes || H * W * 3 > buf_bytes - off) return CODETR_E_BADARG;  // the image lies in the buffer
    tab->img[n].offset = off, tab->img[n].H = (int)H, tab->img[n].W = (int)W;
    *Wmax = W > *Wmax ? W : *Wmax;
  }
  return 0;
}

}  // namespace crops_args
