// Lens undistortion on the GPU (include/codetr_undistort.h states the rule): the stored packed RGB frames of a chunk --
// what frames_to_rgb_kernel, raw_to_rgb_kernel and the JPEG decoder leave -- remapped through OpenCV's rational (Brown)
// or fisheye model into the rectilinear images every later kernel reads.  A data-dependent gather: the tile schemes of
// frames.hip, orient.hip, raw.hip and crops.hip know their source rectangle before they look at a pixel, this one has to
// compute it.
//
// undistort_rgb_kernel  grid (ceil(W'max / 64), ceil(H'max / 16), N), 256 threads; the frame's table entry, its sixteen
//                     parameters included, is a kernel argument read with a uniform index, and the model is uniform per
//                     workgroup, so its branch diverges nowhere.  A workgroup owns a 64 x 16 tile of OUTPUT pixels --
//                     wider than high, so that an output row leaves as 192 consecutive bytes --, a thread one group of
//                     4 consecutive pixels: tile row tid >> 4, pixels 4 (tid & 15) .. + 3, packed to three dwords where
//                     the address is 4-byte aligned and written byte by byte otherwise, as orient.hip does.
//   coordinates       computed on the fly (steps 1-3 of the rule, about 40 fp32 operations per pixel for brown, 60 for
//                     fisheye with its two divisions and a root), once per pixel, kept in registers as (X, Y).  A stored
//                     per-camera map would be read at 8 bytes per output pixel, more than the 3 + 3 bytes the image itself
//                     moves, and would need a cache keyed by camera; the arithmetic keeps the stage stateless, so a launch
//                     may mix cameras freely.  Priced, not measured.
//   source window     the four taps of a pixel overlap those of its neighbours.  The workgroup reduces min / max of (xi,
//                     yi) over its pixels that have at least one tap inside the frame (shuffles inside a wave, then 16
//                     words of LDS) and, when the bounding window (xmax - xmin + 2) x (ymax - ymin + 2) fits, stages it in
//                     LDS as one dword per pixel (R | G << 8 | B << 16) with `fill` at the positions outside the frame,
//                     so that the sampler tests no bounds.  A window row is read in groups of 4 pixels that start at x ==
//                     (row address) mod 4, which is where 3 x bytes behind the row's first byte is 4-byte aligned: whatever
//                     the offset and pitch, every group inside the frame is three aligned dwords, and only the groups that
//                     straddle the frame's left or right edge go byte by byte.  After one barrier every pixel reads
//                     its four taps from LDS.
//   LDS budget        4864 dwords of window + 16 words = 19520 bytes per workgroup: 8 workgroups per CU (156160 of 163840
//                     bytes), which is the wave limit (32 waves per CU, 4 per workgroup).  A mild calibration needs 66 x 18
//                     = 1188 dwords; the budget holds a tile whose source is 2 x 2 times as large (130 x 34).
//   window pitch      ww | 1 dwords, ww = xmax - xmin + 2.  Model (the one tests/test_lds_bank_model.py uses): 64 banks of 4
//                     bytes, bank = dword address mod 64.  A tap read is one dword per lane; a wave holds 4 tile rows of
//                     16 lanes, and at unit magnification lane (r, l) reads dword pitch (y0 + r) + x0 + 4 l + i: two lanes
//                     meet in a bank iff pitch (r - r') == 4 (l' - l) mod 64, which needs pitch (r - r') == 0 mod 4, and
//                     an odd pitch with |r - r'| < 4 allows that for r = r' only -- where 4 (l' - l) covers 16 different
//                     banks.  So the read is conflict-free at unit magnification for every odd pitch, and an even ww is
//                     padded by one dword.  Away from unit magnification the addresses are the lens's and no pitch can
//                     promise anything; magnifications near 1 are what a calibration produces.  (The staging writes put
//                     consecutive groups 4 dwords apart: a wave covers 256 dwords of a row, 4 lanes per bank where a window
//                     row is that long; a row of a mild window has 17 groups and the next row starts an odd pitch on.)
//   direct path       a window over budget -- a strong zoom-out, a tile in the far field of a fisheye -- is not staged: the
//                     same arithmetic, taps read from global memory with bounds tests.  The choice is uniform per
//                     workgroup and both paths feed one blend function, so they give the same bytes.
// Nothing outside a declared source row is read and nothing outside an output image is written.  No scratch.
// A translation unit of its own on purpose: the code of frames.hip, orient.hip and raw.hip is pinned.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_undistort.h"
#include "undistort_args.h"

// fp32 with one rounding per operation: contraction is off for the whole file, divisions and roots are IEEE.
#pragma clang fp contract(off)

namespace {

using undistort::Image;
using undistort::ImageTable;

constexpr int kTileW = 64, kTileH = 16;  // output pixels per tile
constexpr int kPix = 4;                  // pixels per group
constexpr int kThreads = 256;            // one group per thread
constexpr int kWinDwords = 4864;         // the staged window's budget

typedef unsigned u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// 4 pixels at the 4-byte aligned p -> one dword per pixel; reads exactly 12 bytes
__device__ __forceinline__ void load_group(const unsigned char* __restrict__ p, unsigned (&px)[kPix]) {
  const u32x3_a4 v = *reinterpret_cast<const u32x3_a4*>(p);
  px[0] = v.x & 0xFFFFFFu;
  px[1] = (v.x >> 24 | v.y << 8) & 0xFFFFFFu;
  px[2] = (v.y >> 16 | v.z << 16) & 0xFFFFFFu;
  px[3] = v.z >> 8;
}

__device__ __forceinline__ unsigned load_pixel(const unsigned char* __restrict__ p) {
  return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
}

// npx (1..4) pixels, one dword each (the top byte zero) -> 3 npx bytes at q
__device__ __forceinline__ void store_group(unsigned char* __restrict__ q, int npx, const unsigned (&px)[kPix]) {
  if (npx == kPix && aligned4(q)) {
    u32x3_a4 o;
    o.x = px[0] | px[1] << 24;
    o.y = px[1] >> 8 | px[2] << 16;
    o.z = px[2] >> 16 | px[3] << 8;
    *reinterpret_cast<u32x3_a4*>(q) = o;
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      if (i < npx) {
        q[3 * i] = (unsigned char)px[i];
        q[3 * i + 1] = (unsigned char)(px[i] >> 8);
        q[3 * i + 2] = (unsigned char)(px[i] >> 16);
      }
    }
  }
}

// the header's ATAN: r >= 0
__device__ __forceinline__ float atan_rule(float r) {
  const bool inv = r > 1.0f;
  const float z = inv ? 1.0f / r : r;
  const float w = z * z;
  float p = -0x1.1d6f08p-8f;
  p = 0x1.797cd6p-6f + w * p;
  p = -0x1.d947a4p-5f + w * p;
  p = 0x1.912bdep-4f + w * p;
  p = -0x1.1e3d86p-3f + w * p;
  p = 0x1.98d60ep-3f + w * p;
  p = -0x1.5550f2p-2f + w * p;
  p = 1.0f + w * p;
  const float q = z * p;
  return inv ? 0x1.921fb6p+0f - q : q;
}

// steps 1-3 for output pixel (u, v): false where the pixel is `fill`
template <bool kFisheye>
__device__ __forceinline__ bool source_position(const Image& im, int u, int v, int& X, int& Y) {
  const float* __restrict__ k = im.p + 8;
  const float x = ((float)u - im.p[6]) / im.p[4], y = ((float)v - im.p[7]) / im.p[5];
  const float xx = x * x, yy = y * y, r2 = xx + yy;
  float xd, yd;
  if (kFisheye) {
    const float r = __builtin_sqrtf(r2);  // (the correctly rounded sequence)
    const float t = atan_rule(r), t2 = t * t;
    const float td = t * (1.0f + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
    const float s = r2 == 0.0f ? 1.0f : td / r;
    xd = x * s, yd = y * s;
  } else {
    const float num = 1.0f + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
    const float den = 1.0f + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
    const float kr = num / den, xy = x * y;
    xd = ((x * kr) + ((k[2] + k[2]) * xy)) + (k[3] * (r2 + (xx + xx)));
    yd = ((y * kr) + ((k[3] + k[3]) * xy)) + (k[2] * (r2 + (yy + yy)));
  }
  const float us = (im.p[0] * xd) + im.p[2], vs = (im.p[1] * yd) + im.p[3];
  const float fX = floorf((us * 32.0f) + 0.5f), fY = floorf((vs * 32.0f) + 0.5f);
  if (!(fX >= -1048576.0f && fX <= 1048576.0f && fY >= -1048576.0f && fY <= 1048576.0f)) return false;  // (a NaN fails)
  X = (int)fX, Y = (int)fY;
  return true;
}

// step 4's blend of four taps (one dword per pixel), a = X & 31, b = Y & 31
__device__ __forceinline__ unsigned blend(unsigned p00, unsigned p01, unsigned p10, unsigned p11, int a, int b) {
  const unsigned w00 = (32 - a) * (32 - b), w01 = a * (32 - b), w10 = (32 - a) * b, w11 = a * b;
  unsigned out = 0;
#pragma unroll
  for (int sh = 0; sh < 24; sh += 8) {
    const unsigned v = w00 * (p00 >> sh & 255u) + w01 * (p01 >> sh & 255u) + w10 * (p10 >> sh & 255u) + w11 * (p11 >> sh & 255u);
    out |= (v + 512u) >> 10 << sh;
  }
  return out;
}

// a tap of the direct path: the stored pixel, or `fill` outside the frame
__device__ __forceinline__ unsigned tap(const unsigned char* __restrict__ s, const Image& im, int y, int x) {
  if ((unsigned)y >= (unsigned)im.H || (unsigned)x >= (unsigned)im.W) return im.fill;
  return load_pixel(s + (int64_t)y * im.pitch + (int64_t)x * 3);
}

// grid (ceil(W'max / 64), ceil(H'max / 16), N)
__global__ __launch_bounds__(kThreads) void undistort_rgb_kernel(const unsigned char* __restrict__ src, ImageTable tab,
                                                                 unsigned char* __restrict__ dst) {
  __shared__ unsigned sm[kWinDwords];
  __shared__ int red[kThreads / 64][4];
  const Image& im = tab.f[blockIdx.z];  // (uniform: the entry comes through the scalar cache)
  const int H = im.H, W = im.W, Ho = im.Ho, Wo = im.Wo;
  const int ty = blockIdx.y * kTileH, tx = blockIdx.x * kTileW;
  if (ty >= Ho || tx >= Wo) return;  // (uniform)
  const unsigned char* __restrict__ s = src + im.src;
  const int v = ty + (threadIdx.x >> 4), u0 = tx + (threadIdx.x & 15) * kPix;
  const int npx = v < Ho ? max(0, min(kPix, Wo - u0)) : 0;  // this thread's pixels inside the image

  // steps 1-3; `live` marks the pixels with at least one tap inside the frame -- the others are `fill`
  int X[kPix], Y[kPix];
  unsigned live = 0;
  int xmin = INT_MAX, xmax = INT_MIN, ymin = INT_MAX, ymax = INT_MIN;
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    X[i] = 0, Y[i] = 0;
    if (i >= npx) continue;
    const bool ok = im.model == CODETR_UNDISTORT_FISHEYE ? source_position<true>(im, u0 + i, v, X[i], Y[i])
                                                         : source_position<false>(im, u0 + i, v, X[i], Y[i]);
    const int xi = X[i] >> 5, yi = Y[i] >> 5;
    if (ok && xi >= -1 && xi < W && yi >= -1 && yi < H) {
      live |= 1u << i;
      xmin = min(xmin, xi), xmax = max(xmax, xi), ymin = min(ymin, yi), ymax = max(ymax, yi);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    xmin = min(xmin, __shfl_xor(xmin, m)), xmax = max(xmax, __shfl_xor(xmax, m));
    ymin = min(ymin, __shfl_xor(ymin, m)), ymax = max(ymax, __shfl_xor(ymax, m));
  }
  if ((threadIdx.x & 63) == 0) {
    int* r = red[threadIdx.x >> 6];
    r[0] = xmin, r[1] = xmax, r[2] = ymin, r[3] = ymax;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    xmin = min(xmin, red[w][0]), xmax = max(xmax, red[w][1]);
    ymin = min(ymin, red[w][2]), ymax = max(ymax, red[w][3]);
  }
  // (uniform from here) the window [xmin, xmax + 1] x [ymin, ymax + 1]: sides <= 32769, the product fits an int
  const bool any = xmin <= xmax;
  const int ww = any ? xmax - xmin + 2 : 0, wh = any ? ymax - ymin + 2 : 0, pitch = ww | 1;
  const bool staged = any && pitch * wh <= kWinDwords;

  if (staged) {
    const int G = (ww + 6) >> 2;  // groups per window row: the first starts up to 3 pixels left of xmin
    for (int idx = threadIdx.x; idx < wh * G; idx += kThreads) {
      const int wy = idx / G, g = idx - wy * G;
      const int ys = ymin + wy;
      const bool row_in = (unsigned)ys < (unsigned)H;
      const unsigned char* __restrict__ rowp = s + (int64_t)(row_in ? ys : 0) * im.pitch;
      const int phase = (int)((uintptr_t)rowp & 3u);          // pixels x == phase (mod 4) lie at 4-byte aligned addresses
      const int gx = xmin - ((xmin - phase) & 3) + 4 * g;
      unsigned px[kPix] = {im.fill, im.fill, im.fill, im.fill};
      if (row_in) {
        if (gx >= 0 && gx + kPix <= W) {
          load_group(rowp + (int64_t)gx * 3, px);
        } else {
#pragma unroll
          for (int i = 0; i < kPix; ++i)
            if ((unsigned)(gx + i) < (unsigned)W) px[i] = load_pixel(rowp + (int64_t)(gx + i) * 3);
        }
      }
#pragma unroll
      for (int i = 0; i < kPix; ++i) {
        const int lx = gx + i - xmin;
        if ((unsigned)lx < (unsigned)ww) sm[wy * pitch + lx] = px[i];
      }
    }
    __syncthreads();
  }

  if (npx == 0) return;
  unsigned out[kPix];
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    out[i] = im.fill;
    if (!(live >> i & 1u)) continue;
    const int xi = X[i] >> 5, yi = Y[i] >> 5, a = X[i] & 31, b = Y[i] & 31;
    if (staged) {
      const unsigned* __restrict__ w = sm + (yi - ymin) * pitch + (xi - xmin);  // all four inside the window
      out[i] = blend(w[0], w[1], w[pitch], w[pitch + 1], a, b);
    } else {
      out[i] = blend(tap(s, im, yi, xi), tap(s, im, yi, xi + 1), tap(s, im, yi + 1, xi), tap(s, im, yi + 1, xi + 1), a, b);
    }
  }
  store_group(dst + im.dst + ((int64_t)v * Wo + u0) * 3, npx, out);
}

}  // namespace

extern "C" int codetr_undistort_abi_version(void) { return CODETR_UNDISTORT_ABI_VERSION; }

extern "C" int codetr_undistort_rgb_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host,
                                       const float* params_host, void* dst_dev, int64_t dst_bytes) {
  ImageTable tab = {};
  int64_t Hmax = 0, Wmax = 0;  // of the output images
  const int rc = undistort::check((uintptr_t)src_dev, src_bytes, N, rows_host, params_host, (uintptr_t)dst_dev, dst_bytes, &tab,
                                  &Hmax, &Wmax);
  if (rc != 0) return rc;
  const dim3 grid((unsigned)((Wmax + kTileW - 1) / kTileW), (unsigned)((Hmax + kTileH - 1) / kTileH), (unsigned)N);
  hipLaunchKernelGGL(undistort_rgb_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned char*>(src_dev), tab, static_cast<unsigned char*>(dst_dev));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}
