// The object crops of include/codetr_crops.h: codetr_crop_detections_*.  Two launches on one stream, the images only read.
//
// crop_select_kernel    one 256-thread workgroup per image walks its detection rows 256 at a time.  A thread evaluates one
//                       row (the header's selection and region); the wave's ballot and a prefix over the four wave totals
//                       give the row its slot, so the slots keep the row order without an atomic.  The slot's table entry
//                       (row, region, inner rectangle) and the image's count are all the second launch reads of the
//                       detections.  The walk stops once max_per_img slots are full.
// crop_resample_kernel  grid (bands of kBand output rows, slots, images), 128 threads; a workgroup of a slot beyond its
//                       image's count returns at once.  A ROW STREAM: a region may be reduced 50-fold, so the source
//                       footprint of an output tile fits no LDS -- the band walks the source rows of its footprint once.
//   Stage     a source row's segment x0..x1 comes into LDS as the aligned dwords that cover it (a lane per dword, 128 per
//             round; image offsets and row pitches carry no alignment, so the two end dwords are assembled from their
//             bytes inside the segment -- the idiom of redact.hip).  The LDS row is sized by the launcher from the widest
//             image of the call (dynamic LDS, 49 160 B at the 16 384-pixel limit, 5.8 KiB for a 1080p frame).
//   Lanes     a thread owns the output columns tid, tid + 128, ... (kCols of them: 1 / 2 / 4 for out_w <= 128 / 256 /
//             512) with all three channels.  Its tap range and normaliser per column are loop invariants in registers;
//             the weights are recomputed from integers (one add and one abs-difference per tap), never tabulated.  A
//             column's three channels share the weight, which is why the lane is a column and not a (column, channel).
//   Rows      the row value t (8.8 fixed point) of a column stays in the registers of the thread that made it and is
//             added, times the row's vertical weight, into the kBand output rows the thread holds for that column:
//             kCols x 3 x kBand 64-bit accumulators (48 / 96 / 96 registers: kBand is 8, 8, 4).  The vertical weights
//             are wave-uniform; a source row touches at most two output rows when reducing and up to all of them when
//             enlarging -- the same unrolled loop, predicated on a uniform weight.  Adjacent bands re-read only the
//             rows of the vertical support.
//   Division  t = (hs * 256 + Nrm / 2) / Nrm with a per-thread-constant divisor below 2^30 and a numerator below 2^47:
//             one fp64 multiply by the reciprocal and one exact integer correction step instead of a 64-bit division
//             per row, column and channel.
//   Epilogue  (vs + D / 2) / D per output value, pad_rgb outside the inner rectangle, the uint8 HWC slot and, when asked,
//             the normalised CHW slot in the tensor's type.
// fp32 with one rounding per operation: contraction is off for the whole file.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_crops.h"
#include "box_prims.h"
#include "box_region.h"
#include "crops_args.h"

namespace {

using crops_args::Image;
using crops_args::Table;

constexpr int kSelThreads = 256, kThreads = 128, kInts = CODETR_CROPS_TABLE_INTS;
static_assert(kSelThreads == 4 * 64, "four waves: one ballot each");
static_assert(CODETR_CROPS_MAX_SIDE <= 4 * kThreads, "at most four columns per thread");

struct Params {
  int w, h, M, fit, C;
  float score_thr, expand;
  int pad[3];
  int tensor_type;
  float mean[3], stdv[3];
};

// ---- the selection pass: grid (N), 256 threads
template <class T>
__global__ __launch_bounds__(kSelThreads) void crop_select_kernel(Table tab, const T* __restrict__ boxes,
                                                                  const T* __restrict__ scores,
                                                                  const int64_t* __restrict__ labels,
                                                                  const int* __restrict__ count, int Q,
                                                                  const unsigned char* __restrict__ select, Params p,
                                                                  int* __restrict__ table, int* __restrict__ counts) {
  __shared__ int s_wave[4];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Image im = tab.img[n];
  const T* ibox = boxes + (size_t)n * Q * 4;
  const T* iscore = scores + (size_t)n * Q;
  const int64_t* ilabel = labels + (size_t)n * Q;
  const int cnt = min(max(count[n], 0), Q);
  int filled = 0;  // (uniform) candidates so far
  for (int base = 0; base < cnt && filled < p.M; base += kSelThreads) {
    const int j = base + tid;
    bool take = false;
    int4 r = make_int4(0, 0, 0, 0);
    if (j < cnt) {
      const float s = to_f32(iscore[j]);
      const int64_t label = ilabel[j];
      const float x1 = to_f32(ibox[4 * j]), y1 = to_f32(ibox[4 * j + 1]);
      const float x2 = to_f32(ibox[4 * j + 2]), y2 = to_f32(ibox[4 * j + 3]);
      const bool chosen = select == nullptr || (label >= 0 && label < p.C && select[label] != 0);
      if (s >= p.score_thr && chosen && __builtin_isfinite(x1) && __builtin_isfinite(y1) && __builtin_isfinite(x2) &&
          __builtin_isfinite(y2) && region_of(x1, y1, x2, y2, p.expand, &r)) {
        r = make_int4(max(r.x, 0), max(r.y, 0), min(r.z + 1, im.W), min(r.w + 1, im.H));  // half-open, clipped
        take = r.z > r.x && r.w > r.y;
      }
    }
    const unsigned long long votes = __ballot(take);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = filled, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = s_wave[k];
      before += k < wave ? c : 0;
      total += c;
    }
    const int slot = before + __popcll(votes & ((1ull << lane) - 1ull));
    if (take && slot < p.M) {
      int ox, oy, iw, ih;
      crops_args::inner_rect(p.fit, r.z - r.x, r.w - r.y, p.w, p.h, &ox, &oy, &iw, &ih);
      int* e = table + ((size_t)n * p.M + slot) * kInts;
      e[0] = j, e[1] = r.x, e[2] = r.y, e[3] = r.z, e[4] = r.w, e[5] = ox, e[6] = oy, e[7] = iw, e[8] = ih;
      e[9] = e[10] = e[11] = 0;
    }
    filled += total;
    __syncthreads();  // the wave totals are read: the next round may write them
  }
  if (tid == 0) counts[n] = min(filled, p.M);
}

// ---- the resampling kernel
// floor((num) / den) for num < 2^47 and den < 2^30, inv = 1.0 / den: the fp64 estimate is off by at most one
__device__ __forceinline__ unsigned div_floor(unsigned long long num, unsigned den, double inv) {
  unsigned long long q = (unsigned long long)((double)num * inv);
  const long long rem = (long long)num - (long long)(q * den);
  if (rem < 0) --q;
  else if (rem >= (long long)den) ++q;
  return (unsigned)q;
}

template <int kCols, int kBand>
__global__ __launch_bounds__(kThreads) void crop_resample_kernel(const unsigned char* __restrict__ buf, Table tab,
                                                                 const int* __restrict__ table,
                                                                 const int* __restrict__ counts, Params p,
                                                                 unsigned char* __restrict__ crops,
                                                                 void* __restrict__ tensor) {
  extern __shared__ unsigned s_row[];  // the aligned dwords of one source row segment
  const int n = blockIdx.z, slot = blockIdx.y, tid = threadIdx.x;
  if (slot >= counts[n]) return;  // (uniform) a slot beyond the image's count: nothing is written
  const Image im = tab.img[n];
  const int* e = table + ((size_t)n * p.M + slot) * kInts;
  const int x0 = e[1], y0 = e[2], Rw = e[3] - e[1], Rh = e[4] - e[2];
  const int ox = e[5], oy = e[6], iw = e[7], ih = e[8];
  const int r0 = blockIdx.x * kBand;                        // the band's first output row
  const int last = min(r0 + kBand - 1, p.h - 1);            // and its last
  const int jlo = max(r0 - oy, 0), jhi = min(last - oy, ih - 1);  // the inner rows it holds (none: jlo > jhi)

  // the thread's columns: inner index, tap range and normaliser (a column outside the inner rectangle has none)
  int ci[kCols], slo[kCols], shi[kCols];
  unsigned nx[kCols];
  double inv[kCols];
  const int Sx = 2 * max(iw, Rw);
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const int c = tid + k * kThreads;
    ci[k] = c < p.w && c >= ox && c < ox + iw ? c - ox : -1;
    slo[k] = 0, shi[k] = -1, nx[k] = 1;
    if (ci[k] >= 0) {
      crops_args::tap_range(ci[k], iw, Rw, &slo[k], &shi[k]);
      unsigned sum = 0;
      int d = (2 * slo[k] + 1) * iw - (2 * ci[k] + 1) * Rw;
      for (int s = slo[k]; s <= shi[k]; ++s, d += 2 * iw) sum += (unsigned)max(Sx - abs(d), 0);
      nx[k] = sum;
    }
    inv[k] = 1.0 / (double)nx[k];
  }

  unsigned long long acc[kCols][3][kBand];
  unsigned ny[kBand];
#pragma unroll
  for (int r = 0; r < kBand; ++r) {
    ny[r] = 0;
#pragma unroll
    for (int k = 0; k < kCols; ++k) acc[k][0][r] = acc[k][1][r] = acc[k][2][r] = 0;
  }

  if (jlo <= jhi) {  // (uniform) the band holds inner rows: walk the source rows of its footprint once
    int ylo, yhi, unused;
    crops_args::tap_range(jlo, ih, Rh, &ylo, &unused);
    crops_args::tap_range(jhi, ih, Rh, &unused, &yhi);
    const unsigned char* img = buf + im.offset;
    const int Sy = 2 * max(ih, Rh), len = 3 * Rw;
    for (int y = ylo; y <= yhi; ++y) {
      // ---- stage: the aligned dwords that cover the row's segment
      const unsigned char* seg = img + ((int64_t)(y0 + y) * im.W + x0) * 3;
      const int phase = (int)((uintptr_t)seg & 3u), ndw = (phase + len + 3) >> 2;
      for (int dw = tid; dw < ndw; dw += kThreads) {
        const int k0 = 4 * dw - phase;  // the segment byte of the dword's first byte
        unsigned v = 0;
        if (k0 >= 0 && k0 + 4 <= len) {
          v = *reinterpret_cast<const unsigned*>(seg + k0);
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (k0 + b >= 0 && k0 + b < len) v |= (unsigned)seg[k0 + b] << (8 * b);
        }
        s_row[dw] = v;
      }
      __syncthreads();
      // ---- the row's vertical weights for the band's rows (uniform)
      unsigned wy[kBand];
#pragma unroll
      for (int r = 0; r < kBand; ++r) {
        const int j = r0 + r - oy;
        wy[r] = j >= 0 && j < ih && r0 + r < p.h ? (unsigned)max(Sy - abs((2 * y + 1) * ih - (2 * j + 1) * Rh), 0) : 0u;
        ny[r] += wy[r];
      }
      // ---- horizontal pass of the thread's columns, then into the accumulators
      const unsigned char* row = reinterpret_cast<const unsigned char*>(s_row) + phase;
#pragma unroll
      for (int k = 0; k < kCols; ++k) {
        if (ci[k] < 0) continue;
        unsigned long long h0 = 0, h1 = 0, h2 = 0;
        int d = (2 * slo[k] + 1) * iw - (2 * ci[k] + 1) * Rw;
        const unsigned char* px = row + 3 * slo[k];
        for (int s = slo[k]; s <= shi[k]; ++s, d += 2 * iw, px += 3) {
          const unsigned wt = (unsigned)max(Sx - abs(d), 0);
          h0 += (unsigned long long)wt * px[0], h1 += (unsigned long long)wt * px[1], h2 += (unsigned long long)wt * px[2];
        }
        const unsigned half = nx[k] >> 1;
        const unsigned t0 = div_floor(h0 * 256 + half, nx[k], inv[k]), t1 = div_floor(h1 * 256 + half, nx[k], inv[k]);
        const unsigned t2 = div_floor(h2 * 256 + half, nx[k], inv[k]);
#pragma unroll
        for (int r = 0; r < kBand; ++r) {
          if (wy[r] != 0) {  // (uniform)
            acc[k][0][r] += (unsigned long long)wy[r] * t0;
            acc[k][1][r] += (unsigned long long)wy[r] * t1;
            acc[k][2][r] += (unsigned long long)wy[r] * t2;
          }
        }
      }
      __syncthreads();  // the row is read: the next may overwrite it
    }
  }

  // ---- epilogue: the final division, the padding, the uint8 HWC slot and the normalised CHW slot
  const size_t slot_index = (size_t)n * p.M + slot, plane = (size_t)p.h * p.w;
  unsigned char* out = crops + slot_index * plane * 3;
#pragma unroll
  for (int r = 0; r < kBand; ++r) {
    const int orow = r0 + r;
    if (orow >= p.h) break;
    const bool inner_row = orow >= oy && orow < oy + ih;
    const unsigned long long D = (unsigned long long)ny[r] * 256;
#pragma unroll
    for (int k = 0; k < kCols; ++k) {
      const int c = tid + k * kThreads;
      if (c >= p.w) continue;
      int v[3] = {p.pad[0], p.pad[1], p.pad[2]};
      if (inner_row && ci[k] >= 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = (int)((acc[k][ch][r] + (D >> 1)) / D);
      }
      unsigned char* o = out + ((size_t)orow * p.w + c) * 3;
      o[0] = (unsigned char)v[0], o[1] = (unsigned char)v[1], o[2] = (unsigned char)v[2];
      if (p.tensor_type != CODETR_CROPS_TENSOR_NONE) {
        const size_t at = slot_index * 3 * plane + (size_t)orow * p.w + c;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float f = ((float)v[ch] - p.mean[ch]) / p.stdv[ch];
          const size_t i = at + ch * plane;
          if (p.tensor_type == CODETR_CROPS_TENSOR_F32) static_cast<float*>(tensor)[i] = f;
          else if (p.tensor_type == CODETR_CROPS_TENSOR_F16) static_cast<_Float16*>(tensor)[i] = (_Float16)f;
          else static_cast<unsigned short*>(tensor)[i] = bf16_from_f32(f);
        }
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

template <int kCols, int kBand>
void launch_resample(hipStream_t stream, int64_t N, size_t lds, const void* buf, const Table& tab, const int* table,
                     const int* counts, const Params& p, void* crops, void* tensor) {
  const dim3 grid((unsigned)((p.h + kBand - 1) / kBand), (unsigned)p.M, (unsigned)N);
  hipLaunchKernelGGL((crop_resample_kernel<kCols, kBand>), grid, dim3(kThreads), lds, stream,
                     static_cast<const unsigned char*>(buf), tab, table, counts, p, static_cast<unsigned char*>(crops), tensor);
}

template <class T>
int launch_crops(void* stream, const void* buf, int64_t buf_bytes, int64_t N, const int64_t* images, const void* boxes,
                 const void* scores, const int64_t* labels, const int* count, int64_t Q, const unsigned char* select,
                 int64_t C, int out_w, int out_h, int max_per_img, int fit, float score_thr, float expand, uint32_t pad_rgb,
                 void* crops, int* counts, int* table, void* tensor, int tensor_type, const float* mean, const float* stdv) {
  Table tab = {};
  int64_t Wmax = 0;
  const int rc = crops_args::check(buf, buf_bytes, N, images, boxes, scores, labels, count, Q, select, C, out_w, out_h,
                                   max_per_img, fit, score_thr, expand, pad_rgb, crops, counts, table, tensor, tensor_type,
                                   mean, stdv, &tab, &Wmax);
  if (rc != 0) return rc;
  Params p = {};
  p.w = out_w, p.h = out_h, p.M = max_per_img, p.fit = fit, p.C = select ? (int)C : 0;
  p.score_thr = score_thr, p.expand = expand;
  p.pad[0] = (int)((pad_rgb >> 16) & 255u), p.pad[1] = (int)((pad_rgb >> 8) & 255u), p.pad[2] = (int)(pad_rgb & 255u);
  p.tensor_type = tensor_type;
  for (int c = 0; c < 3; ++c) p.mean[c] = tensor_type ? mean[c] : 0.f, p.stdv[c] = tensor_type ? stdv[c] : 1.f;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((crop_select_kernel<T>), dim3((unsigned)N), dim3(kSelThreads), 0, st, tab, static_cast<const T*>(boxes),
                     static_cast<const T*>(scores), labels, count, (int)Q, select, p, table, counts);
  const size_t lds = (size_t)((3 * Wmax + 3 + 3) / 4 + 1) * 4;  // a row segment of the widest image at any byte phase
  if (out_w <= kThreads) launch_resample<1, 8>(st, N, lds, buf, tab, table, counts, p, crops, tensor);
  else if (out_w <= 2 * kThreads) launch_resample<2, 8>(st, N, lds, buf, tab, table, counts, p, crops, tensor);
  else launch_resample<4, 4>(st, N, lds, buf, tab, table, counts, p, crops, tensor);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

extern "C" {

int codetr_crops_abi_version(void) { return CODETR_CROPS_ABI_VERSION; }

#define CODETR_CROPS_ENTRY(SUFFIX, TYPE)                                                                                   \
  int codetr_crop_detections_##SUFFIX(void* stream, const void* buf_dev, int64_t buf_bytes, int64_t N,                    \
                                      const int64_t* images_host, const void* boxes_dev, const void* scores_dev,          \
                                      const int64_t* labels_dev, const int* count_dev, int64_t Q,                         \
                                      const unsigned char* select_dev, int64_t C, int out_w, int out_h, int max_per_img,  \
                                      int fit, float score_thr, float expand, uint32_t pad_rgb, void* crops_dev,          \
                                      int* counts_dev, int* table_dev, void* tensor_dev, int tensor_type,                 \
                                      const float* mean_host, const float* std_host) {                                    \
    return launch_crops<TYPE>(stream, buf_dev, buf_bytes, N, images_host, boxes_dev, scores_dev, labels_dev, count_dev, Q, \
                              select_dev, C, out_w, out_h, max_per_img, fit, score_thr, expand, pad_rgb, crops_dev,        \
                              counts_dev, table_dev, tensor_dev, tensor_type, mean_host, std_host);                        \
  }
CODETR_CROPS_ENTRY(f16, _Float16)
CODETR_CROPS_ENTRY(bf16, Bf16)
CODETR_CROPS_ENTRY(f32, float)
#undef CODETR_CROPS_ENTRY

}  // extern "C"
