// Local contrast enhancement (CLAHE) on the GPU (include/codetr_enhance.h states the rule): the packed RGB frames of a
// chunk, their luma equalised per tile of a gy x gx grid with a clipped histogram, the tiles' tables blended between tile
// centres, the change of luma added to R, G and B.  Two launches per 32 frames; a frame is read twice and written once.
//
// enhance_hist_kernel   grid (S max, gy gx max, N), 256 threads: one workgroup per (frame, tile, slice), a slice being a
//                     band of sr tile rows of about CODETR_ENHANCE_SLICE_PIXELS samples (enhance_args.h), so that eight
//                     1080p frames at 8 x 8 give 2048 workgroups and not 512.
//   reading           a slice is up to two spans of stored columns per row -- the tile's columns inside the frame, and the
//                     columns its padded samples reflect to; a padded ROW is another stored row.  Counting does not care
//                     about order, so a reflected span is read forwards.  A span is walked as (row, group) items: groups
//                     of 4 pixels that start where the row's bytes are 4-byte aligned (x == row address mod 4), three
//                     aligned dwords each, and the ragged heads and tails pixel by pixel.  Luma in registers.
//   counting          every wave owns a private 256-bin histogram in LDS (4 KB per workgroup) and adds with LDS atomics; a
//                     lane first merges equal values among its own 4 pixels, so that a flat region costs one atomic per
//                     lane and group, not four.  What same-address atomics of 64 lanes still cost is measured by
//                     tools/bench_enhance.py on a constant frame.
//   result            after one barrier thread b adds the four waves' bin b and stores it, a plain vector store, into the
//                     slice's own 1 KB slot of the workspace.  No global atomics, no memset: deterministic, and every word
//                     the apply pass reads was written by this launch.
// enhance_apply_kernel  grid (bands max, (gy + 1)(gx + 1) max, N), 256 threads.  The image is cut along the lattice of
//                     tile centres: inside one cell (cj, ci) every pixel blends the same four tables (two on an edge, one
//                     in a corner, where the clamped indices coincide).  A cell is at most th x tw and is cut into bands of
//                     br rows for parallelism.
//   tables            thread b owns bin b of the cell's four tables: it adds the slices' partial histograms (coalesced
//                     1 KB rows out of L2; a table that repeats is copied, not read again), clips, and the excess is
//                     reduced over the workgroup (wave shuffles, then 16 words of LDS).  Redistribution is the header's
//                     closed form, per bin.  The inclusive scan over 256 bins is a wave scan on the DPP path (row_shr 1, 2,
//                     4, 8 inside rows of 16 lanes, then the three row totals by v_readlane) plus the totals of the waves in
//                     front through LDS.  Then the division by T.  Two barriers for the tables, a third before the pixels.
//   lookup            the four tables interleaved: the entries for luma v are the four bytes of the dword lut[v] (1 KB), so
//                     a pixel costs one ds_read_b32.  Lanes of a wave read arbitrary dwords of a 256-dword table: 64 banks
//                     (the model of tests/test_lds_bank_model.py) see up to 4 different dwords each in the worst case
//                     and one in a flat region, where all lanes read the same address (a broadcast).
//   pixels            (row, group) items as in the histogram pass: three dwords in, per pixel luma, lookup, the blend in
//                     32-bit integers, the division by 4 T as a multiplication by the host's M = floor(2^32 / 4 T) and one
//                     correction (proved in the header), the shift and clamp, three dwords out where the destination is
//                     4-byte aligned and bytes otherwise; ragged heads and tails pixel by pixel.  Every pixel is read and
//                     written by the one thread whose item holds it, so src == dst is safe.
// Nothing outside a declared source row is read and nothing outside an image's destination rows is written.  No scratch.
// A translation unit of its own on purpose: the code of frames.hip, orient.hip and raw.hip is pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_enhance.h"
#include "device_prims.h"
#include "enhance_args.h"

namespace {

using enhance::Image;
using enhance::ImageTable;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kPix = 4;  // pixels per group

typedef unsigned u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// 4 pixels at the 4-byte aligned p -> one dword per pixel (R | G << 8 | B << 16); reads exactly 12 bytes
__device__ __forceinline__ void load_group(const unsigned char* p, unsigned (&px)[kPix]) {
  const u32x3_a4 v = *reinterpret_cast<const u32x3_a4*>(p);
  px[0] = v.x & 0xFFFFFFu;
  px[1] = (v.x >> 24 | v.y << 8) & 0xFFFFFFu;
  px[2] = (v.y >> 16 | v.z << 16) & 0xFFFFFFu;
  px[3] = v.z >> 8;
}

__device__ __forceinline__ unsigned load_pixel(const unsigned char* p) {
  return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
}

// step 2 of the rule
__device__ __forceinline__ unsigned luma(unsigned px) {
  return (77u * (px & 255u) + 150u * (px >> 8 & 255u) + 29u * (px >> 16) + 128u) >> 8;
}

// the pixels [gx, gx + 4) of the row at `rowp` that lie in [xa, xb): true when all four do (then read as three dwords)
__device__ __forceinline__ bool load_item(const unsigned char* rowp, int gx, int xa, int xb, unsigned (&px)[kPix]) {
  if (gx >= xa && gx + kPix <= xb) {
    load_group(rowp + (int64_t)gx * 3, px);
    return true;
  }
#pragma unroll
  for (int i = 0; i < kPix; ++i) px[i] = gx + i >= xa && gx + i < xb ? load_pixel(rowp + (int64_t)(gx + i) * 3) : 0u;
  return false;
}

// the first group of a row's span [xa, ..): at or up to 3 pixels left of xa, where the row's bytes are 4-byte aligned
__device__ __forceinline__ int first_group(const unsigned char* rowp, int xa) {
  const int phase = (int)((uintptr_t)rowp & 3u);  // pixels x == phase (mod 4) lie at 4-byte aligned addresses
  return xa - ((xa - phase) & 3);
}

// the lumas of the stored columns [xa, xb) of the padded rows [py, py + nrows) counted into the wave's histogram `h`
__device__ __forceinline__ void count_span(const unsigned char* __restrict__ s, const Image& im, int py, int nrows, int xa,
                                           int xb, unsigned* h) {
  if (xa >= xb) return;             // (uniform)
  const int G = (xb - xa + 6) >> 2;  // groups per row: the first starts up to 3 pixels left of xa
  for (int idx = threadIdx.x; idx < nrows * G; idx += kThreads) {
    const int r = idx / G, g = idx - r * G;
    int y = py + r;
    y = y < im.H ? y : 2 * (im.H - 1) - y;  // step 3
    const unsigned char* __restrict__ rowp = s + (int64_t)y * im.spitch;
    const int gx = first_group(rowp, xa) + kPix * g;
    unsigned px[kPix];
    const bool whole = load_item(rowp, gx, xa, xb, px);
    int v[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) v[i] = whole || (gx + i >= xa && gx + i < xb) ? (int)luma(px[i]) : -1 - i;
    // equal values merged: the first of them adds their number (a pixel outside the span has a value of its own, < 0)
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      bool first = v[i] >= 0;
      unsigned c = 1;
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        if (j < i) first = first && v[j] != v[i];
        if (j > i) c += v[j] == v[i];
      }
      if (first) atomicAdd(&h[v[i]], c);
    }
  }
}

// grid (S max, gy gx max, N)
__global__ __launch_bounds__(kThreads) void enhance_hist_kernel(const unsigned char* __restrict__ src, ImageTable tab,
                                                               unsigned* __restrict__ ws) {
  __shared__ unsigned hist[kWaves][256];
  const Image& im = tab.f[blockIdx.z];  // (uniform: the entry comes through the scalar cache)
  const int sl = blockIdx.x, tile = blockIdx.y;
  if (sl >= im.S || tile >= im.gy * im.gx) return;  // (uniform)
#pragma unroll
  for (int w = 0; w < kWaves; ++w) hist[w][threadIdx.x] = 0;
  __syncthreads();
  const int j = tile / im.gx, i = tile - j * im.gx;
  const int r0 = sl * im.sr, nrows = min(im.sr, im.th - r0);  // >= 1: S = ceil(th / sr)
  const int p0 = i * im.tw, p1 = p0 + im.tw, W = im.W;        // the tile's padded columns
  const unsigned char* __restrict__ s = src + im.src;
  unsigned* h = hist[threadIdx.x >> 6];
  count_span(s, im, j * im.th + r0, nrows, min(p0, W), min(p1, W), h);
  // padded columns p in [max(p0, W), p1) read column 2 (W - 1) - p, which is in 0..W - 2 (header, step 3)
  const int q0 = max(p0, W);
  if (q0 < p1) count_span(s, im, j * im.th + r0, nrows, 2 * (W - 1) - (p1 - 1), 2 * (W - 1) - q0 + 1, h);
  __syncthreads();
  unsigned sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) sum += hist[w][threadIdx.x];
  ws[((size_t)im.base + (size_t)tile * im.S + sl) * 256 + threadIdx.x] = sum;
}

template <int CTRL>
__device__ __forceinline__ unsigned add_shifted(unsigned v) { return v + dpp_u<CTRL>(v); }  // (lanes shifted in from outside a row: 0)

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ unsigned wave_scan(unsigned v) {
  v = add_shifted<0x111>(v);  // row_shr:1
  v = add_shifted<0x112>(v);  // row_shr:2
  v = add_shifted<0x114>(v);  // row_shr:4
  v = add_shifted<0x118>(v);  // row_shr:8 -- now inclusive inside each row of 16 lanes
  const unsigned t0 = (unsigned)__builtin_amdgcn_readlane((int)v, 15), t1 = (unsigned)__builtin_amdgcn_readlane((int)v, 31),
                 t2 = (unsigned)__builtin_amdgcn_readlane((int)v, 47);
  const int row = (threadIdx.x & 63) >> 4;
  return v + (row >= 1 ? t0 : 0u) + (row >= 2 ? t1 : 0u) + (row >= 3 ? t2 : 0u);
}

// bin threadIdx.x of a tile's histogram: its slices' partials added
__device__ __forceinline__ unsigned tile_bin(const unsigned* __restrict__ ws, const Image& im, int j, int i) {
  const unsigned* __restrict__ p = ws + ((size_t)im.base + (size_t)(j * im.gx + i) * im.S) * 256 + threadIdx.x;
  unsigned a = 0;
  for (int s = 0; s < im.S; ++s) a += p[(size_t)s * 256];
  return a;
}

// grid (bands max, (gy + 1)(gx + 1) max, N); src and dst may be one buffer
__global__ __launch_bounds__(kThreads) void enhance_apply_kernel(const unsigned char* src, ImageTable tab,
                                                                const unsigned* __restrict__ ws, unsigned char* dst) {
  __shared__ unsigned lut[256];
  __shared__ unsigned excess[kWaves][4], total[kWaves][4];
  const Image& im = tab.f[blockIdx.z];
  const int band = blockIdx.x, cell = blockIdx.y;
  const int gy = im.gy, gx = im.gx, th = im.th, tw = im.tw;
  if (band >= im.bands || cell >= (gy + 1) * (gx + 1)) return;  // (uniform)
  // the cell's pixels are those with jy == cj - 1 and ix == ci - 1 (step 7): 2 th (cj - 1) <= 2 y + 1 - th < 2 th cj
  const int cj = cell / (gx + 1), ci = cell - cj * (gx + 1);
  const int ya = cj == 0 ? 0 : ((2 * cj - 1) * th) >> 1, yb = min(im.H, ((2 * cj + 1) * th) >> 1);
  const int xa = ci == 0 ? 0 : ((2 * ci - 1) * tw) >> 1, xb = min(im.W, ((2 * ci + 1) * tw) >> 1);
  const int y0 = ya + band * im.br, y1 = min(yb, y0 + im.br);
  if (y0 >= y1 || xa >= xb) return;  // (uniform)

  // ---- the four tables (j0, i0), (j0, i1), (j1, i0), (j1, i1), bin threadIdx.x of each
  const int j0 = max(cj - 1, 0), j1 = min(cj, gy - 1), i0 = max(ci - 1, 0), i1 = min(ci, gx - 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned h[4], e[4];
  h[0] = tile_bin(ws, im, j0, i0);
  h[1] = i1 != i0 ? tile_bin(ws, im, j0, i1) : h[0];
  h[2] = j1 != j0 ? tile_bin(ws, im, j1, i0) : h[0];
  h[3] = j1 != j0 ? (i1 != i0 ? tile_bin(ws, im, j1, i1) : h[2]) : h[1];
  const unsigned C = im.C, T = im.T;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // step 5: clip, the excess added up over the workgroup
    e[k] = h[k] > C ? h[k] - C : 0u;
    h[k] = min(h[k], C);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) e[k] += __shfl_xor(e[k], m);
    if (lane == 0) excess[wave][k] = e[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned E = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) E += excess[w][k];
    const unsigned r = E & 255u;
    h[k] += E >> 8;
    if (r != 0) {  // the closed form of the residual loop
      const unsigned s = 256u / r;
      h[k] += threadIdx.x % s == 0 && threadIdx.x / s < r;
    }
    h[k] = wave_scan(h[k]);  // step 6
    if (lane == 63) total[wave][k] = h[k];
  }
  __syncthreads();
  unsigned entry = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned cum = h[k];
#pragma unroll
    for (int w = 0; w < kWaves - 1; ++w) cum += w < wave ? total[w][k] : 0u;
    entry |= ((255u * cum + (T >> 1)) / T) << (8 * k);
  }
  lut[threadIdx.x] = entry;
  __syncthreads();

  // ---- the band's pixels
  const unsigned th2 = 2u * th, tw2 = 2u * tw, d = 4u * T, M = im.M;
  const int G = (xb - xa + 6) >> 2, rows = y1 - y0;
  for (int idx = threadIdx.x; idx < rows * G; idx += kThreads) {
    const int r = idx / G, g = idx - r * G, y = y0 + r;
    const unsigned char* sp = src + im.src + (int64_t)y * im.spitch;
    unsigned char* dp = dst + im.dst + (int64_t)y * im.dpitch;
    const int x0 = first_group(sp, xa) + kPix * g;
    const unsigned wy = (unsigned)(2 * y + 1 - th - 2 * th * (cj - 1));  // in [0, 2 th)
    unsigned px[kPix];
    const bool whole = load_item(sp, x0, xa, xb, px);
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const int x = x0 + i;
      if (!whole && (x < xa || x >= xb)) continue;
      const unsigned wx = (unsigned)(2 * x + 1 - tw - 2 * tw * (ci - 1));  // in [0, 2 tw)
      const unsigned v = luma(px[i]), t = lut[v];
      const unsigned top = (tw2 - wx) * (t & 255u) + wx * (t >> 8 & 255u), bot = (tw2 - wx) * (t >> 16 & 255u) + wx * (t >> 24);
      const unsigned n = (th2 - wy) * top + wy * bot + 2u * T;
      unsigned q = __umulhi(n, M);  // floor(n / d) or one less (header)
      q += n - q * d >= d;
      const int shift = (int)q - (int)v;  // step 8
      const int R = min(max((int)(px[i] & 255u) + shift, 0), 255), Gc = min(max((int)(px[i] >> 8 & 255u) + shift, 0), 255),
                B = min(max((int)(px[i] >> 16) + shift, 0), 255);
      px[i] = (unsigned)R | (unsigned)Gc << 8 | (unsigned)B << 16;
    }
    unsigned char* q4 = dp + (int64_t)x0 * 3;
    if (whole && aligned4(q4)) {
      u32x3_a4 o;
      o.x = px[0] | px[1] << 24;
      o.y = px[1] >> 8 | px[2] << 16;
      o.z = px[2] >> 16 | px[3] << 8;
      *reinterpret_cast<u32x3_a4*>(q4) = o;
    } else {
#pragma unroll
      for (int i = 0; i < kPix; ++i) {
        if (x0 + i >= xa && x0 + i < xb) {
          q4[3 * i] = (unsigned char)px[i];
          q4[3 * i + 1] = (unsigned char)(px[i] >> 8);
          q4[3 * i + 2] = (unsigned char)(px[i] >> 16);
        }
      }
    }
  }
}

}  // namespace

extern "C" int codetr_enhance_abi_version(void) { return CODETR_ENHANCE_ABI_VERSION; }

extern "C" int64_t codetr_enhance_workspace_bytes(int64_t N, const int64_t* rows_host) { return enhance::workspace_bytes(N, rows_host); }

extern "C" int codetr_enhance_rgb_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host,
                                     void* dst_dev, int64_t dst_bytes, void* ws_dev, int64_t ws_bytes) {
  ImageTable tab = {};
  enhance::Launch g;
  const int rc = enhance::check((uintptr_t)src_dev, src_bytes, N, rows_host, (uintptr_t)dst_dev, dst_bytes, (uintptr_t)ws_dev, ws_bytes,
                                &tab, &g);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(enhance_hist_kernel, dim3((unsigned)g.slices, (unsigned)g.tiles, (unsigned)N), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned char*>(src_dev), tab, static_cast<unsigned*>(ws_dev));
  hipLaunchKernelGGL(enhance_apply_kernel, dim3((unsigned)g.bands, (unsigned)g.cells, (unsigned)N), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned char*>(src_dev), tab,
                     static_cast<const unsigned*>(ws_dev), static_cast<unsigned char*>(dst_dev));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}
