// Pre- and post-processing either side of CoDETR.forward, on the GPU.
//
// preprocess_kernel   replaces the reference Inferencer's CPU pipeline per image (codetr/inferencer.py:439-452 ->
//                     mmdet Resize(keep_ratio) = cv2.resize(INTER_LINEAR) on uint8, mmdet Pad(size, pad_val),
//                     DetDataPreprocessor (x - mean) / std in fp32, cast to the model dtype) and the mask loop of
//                     run_inference (codetr/inferencer.py:354-358): uint8 HWC RGB in, normalised CHW + mask out.
//                     The resize is OpenCV's 8-bit arithmetic (11-bit fixed-point coefficients, cvRound, edge clamp,
//                     (.. + 2^21) >> 22), so the result is the integer image cv2 would produce, then one fp32
//                     subtract and one IEEE divide per value.  Byte work: one thread per output pixel.
// batched_nms_kernel  replaces torchvision.ops.batched_nms in postprocess_predictions (codetr/inferencer.py:388-398)
//                     for the <= 300 detections of an image: greedy, per class, candidates in descending score order
//                     (the caller passes them sorted), IoU > thr suppresses; fp32 arithmetic on the given boxes.
// preprocess_batch_kernel  the same per-pixel work for up to 32 images of different sizes in one launch, written into
//                     one stacked batch [N, 3, H, W] whose margin beyond each image's Pad region holds the raw
//                     DetDataPreprocessor pad_value (mmdet stack_batch); the per-image table travels in the kernargs.
// postprocess_kernel  postprocess_predictions + the rescale of run_inference (codetr/inferencer.py:343-400) for a
//                     batch, one workgroup per image: score threshold at the storage precision, stable descending sort
//                     (bitonic, index tie-break), the NMS of batched_nms_kernel, boxes / scale factor, compacted output.
// postprocess_softnms_kernel  the same place in the pipeline with the post-processing the model configs ask for
//                     (configs/co_dino_5scale_r50_lsj_8xb2_1x_coco.py:80: max_per_img=300, nms type 'soft_nms'): mmcv's
//                     soft-NMS, methods linear and naive, per class, then the max_per_img cut.  Classes are independent,
//                     so after one sort by label every wave runs the greedy chains of whole classes on its own, without
//                     a workgroup barrier per pick; a second sort orders the emitted detections by decayed score.
// preprocess_views_kernel  preprocess_batch_kernel with a mirror bit per row: test-time augmentation's flipped views
//                     (mmdet RandomFlip runs after Resize and before the padding, so the image is mirrored inside its
//                     resized width and the padding stays on the right); rows may read the same source image.
// tta_merge_kernel    mmdet DetTTAModel._merge_single_sample for up to 4096 candidates per image: the views' detections
//                     un-flipped and concatenated, per-class hard or soft NMS (label segments, one wave per chain, 64
//                     positions per lane), sorted by score, cut to max_per_img.
// preprocess_tiles_kernel  preprocess_batch_kernel with a crop rectangle per row: sliced inference's tiles (SAHI's slicing:
//                     every tile of an image is resized as an image of its own); rows read windows of one uploaded image.
// slice_merge_kernel  the fusion of the tiles' detections, up to 4096 candidates per image: shifted by the tile's origin,
//                     clipped to the image, then greedy per-label (or class-agnostic) NMS or non-maximum merging under
//                     IoU or IoS (intersection over the smaller area), sorted by score, cut to max_per_img.
// wbf_merge_kernel    weighted boxes fusion (include/codetr_wbf.h) over the operands and the front end of tta_merge_kernel:
//                     per label the candidates join, in descending confidence, the cluster whose fused box they overlap
//                     most, or found one; every cluster emits its confidence-weighted mean box and its votes.
// The merge and soft-NMS kernels are their own front ends over ONE set of device functions: pack_key (the tie rule), bitonic_desc
// (either key layout), block_scan / block_sum / block_max_u64, segment_starts, run_segments (the greedy chain with both
// threshold rules) and write_row / zero_row.  postprocess_kernel and the kernels above it are on the Inferencer's default
// path, whose machine code is pinned: postprocess_kernel keeps its own sort, scan and epilogue.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_wbf.h"
#include "box_prims.h"
#include "large_lds.h"

namespace {

// fp32 -> the element type (to_f32 and Bf16: box_prims.h); round to nearest even as ATen does, NaN stays NaN
template <class T>
__device__ __forceinline__ T from_f32(float v) {
  return (T)v;
}
template <>
__device__ __forceinline__ Bf16 from_f32<Bf16>(float v) {
  return Bf16{bf16_from_f32(v)};
}

struct ResizeAxis {
  float scale;  // src / dst
  int src, dst;
};

// source index and the weight of the NEXT sample, scaled by 2048 (cv2: cvRound(f * INTER_RESIZE_COEF_SCALE))
__device__ __forceinline__ void coeff(int d, ResizeAxis ax, int& s, int& a1) {
  // cv2: scale = 1. / (dsize / ssize) in double; fx = (float)((dx + 0.5) * scale - 0.5); sx = cvFloor(fx); fx -= sx
  const double scale = 1.0 / ((double)ax.dst / (double)ax.src);
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int i = (int)floorf(f);
  f -= (float)i;
  if (i < 0) {
    i = 0;
    f = 0.f;
  }
  if (i >= ax.src - 1) {
    i = ax.src - 1;
    f = 0.f;
  }
  s = i;
  a1 = (int)rintf(f * 2048.0f);  // round half to even, as cvRound
}

// pixel (y, x) of the cv2-resized image (y < Hr, x < Wr) of a uint8 HWC RGB image [Hs, Ws, 3] whose rows are `pitch`
// pixels apart (a window of a wider image: its neighbours are clamped to the window) -> v[3] in 0..255
__device__ __forceinline__ void resized_pixel(const unsigned char* __restrict__ src, int Hs, int Ws, int pitch, int Hr,
                                              int Wr, int y, int x, int v[3]) {
  int sy, b1, sx, a1;
  coeff(y, ResizeAxis{0.f, Hs, Hr}, sy, b1);
  coeff(x, ResizeAxis{0.f, Ws, Wr}, sx, a1);
  const int sy1 = min(sy + 1, Hs - 1), sx1 = min(sx + 1, Ws - 1);
  const int a0 = 2048 - a1, b0 = 2048 - b1;
  const unsigned char* r0 = src + ((size_t)sy * pitch) * 3;
  const unsigned char* r1 = src + ((size_t)sy1 * pitch) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int top = a0 * r0[sx * 3 + c] + a1 * r0[sx1 * 3 + c];
    const int bot = a0 * r1[sx * 3 + c] + a1 * r1[sx1 * 3 + c];
    const long long acc = (long long)b0 * top + (long long)b1 * bot + (1 << 21);
    int q = (int)(acc >> 22);
    v[c] = q < 0 ? 0 : (q > 255 ? 255 : q);
  }
}
// ... of a contiguous image
__device__ __forceinline__ void resized_pixel(const unsigned char* __restrict__ src, int Hs, int Ws, int Hr, int Wr,
                                              int y, int x, int v[3]) {
  resized_pixel(src, Hs, Ws, Ws, Hr, Wr, y, x, v);
}

// DetDataPreprocessor's (x - mean) / std of a 0..255 value: one fp32 subtract, one IEEE divide
__device__ __forceinline__ float normalise(int v, float mean, float stdv) { return ((float)v - mean) / stdv; }

template <class OutT>
__global__ __launch_bounds__(256) void preprocess_kernel(const unsigned char* __restrict__ src, int Hs, int Ws, int Hr,
                                                         int Wr, int Hp, int Wp, float m0, float m1, float m2, float s0,
                                                         float s1, float s2, int p0, int p1, int p2,
                                                         OutT* __restrict__ dst, OutT* __restrict__ mask) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= Wp) return;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  int v[3] = {p0, p1, p2};
  const bool inside = y < Hr && x < Wr;
  if (inside) resized_pixel(src, Hs, Ws, Hr, Wr, y, x, v);
  const size_t plane = (size_t)Hp * Wp, o = (size_t)y * Wp + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c * plane + o] = (OutT)normalise(v[c], mean[c], stdv[c]);
  if (mask) mask[o] = inside ? (OutT)0.f : (OutT)1.f;
}

// one image of a batched preprocess launch: its bytes at src + src_offset, resized to (Hr, Wr), Pad region (Hp, Wp)
struct BatchImage {
  int64_t src_offset;
  int Hs, Ws, Hr, Wr, Hp, Wp;
};
constexpr int kPreBatchMax = CODETR_PREPROCESS_BATCH_MAX;  // images per launch: the table is a kernel argument (1 KB)
struct BatchTable {
  BatchImage img[kPreBatchMax];
};
struct BatchNorm {
  float mean[3], stdv[3];
  int pad[3];  // the pipeline Pad's pixel value, normalised like the image
  float fill;  // DetDataPreprocessor's pad_value beyond the Pad region (stored as is, not normalised)
};

// grid (ceil(W / 256), H, N): one thread per output pixel of the stacked batch [N, 3, H, W] (+ mask [N, H, W])
template <class OutT>
__global__ __launch_bounds__(256) void preprocess_batch_kernel(const unsigned char* __restrict__ src, BatchTable tab,
                                                               BatchNorm nm, int H, int W, OutT* __restrict__ dst,
                                                               OutT* __restrict__ mask) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  const int n = blockIdx.z;
  if (x >= W) return;
  const BatchImage im = tab.img[n];
  const bool inside = y < im.Hr && x < im.Wr;
  float o[3] = {nm.fill, nm.fill, nm.fill};
  if (y < im.Hp && x < im.Wp) {
    int v[3] = {nm.pad[0], nm.pad[1], nm.pad[2]};
    if (inside) resized_pixel(src + im.src_offset, im.Hs, im.Ws, im.Hr, im.Wr, y, x, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = normalise(v[c], nm.mean[c], nm.stdv[c]);
  }
  const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
  OutT* d = dst + (size_t)n * 3 * plane;
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c * plane + p] = from_f32<OutT>(o[c]);
  if (mask) mask[(size_t)n * plane + p] = from_f32<OutT>(inside ? 0.f : 1.f);
}

// preprocess_batch_kernel with a mirror bit per row (bit n of `flips`; the table holds at most 32 rows): a mirrored row
// reads the resized image right to left inside its resized width -- the Pad region and everything beyond it stay put.
// (Its own body, resize and normalise shared: folding the two kernels into one function changed the batch kernel's code.)
template <class OutT>
__global__ __launch_bounds__(256) void preprocess_views_kernel(const unsigned char* __restrict__ src, BatchTable tab,
                                                               unsigned flips, BatchNorm nm, int H, int W,
                                                               OutT* __restrict__ dst, OutT* __restrict__ mask) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  const int n = blockIdx.z;
  if (x >= W) return;
  const BatchImage im = tab.img[n];
  const bool inside = y < im.Hr && x < im.Wr;
  float o[3] = {nm.fill, nm.fill, nm.fill};
  if (y < im.Hp && x < im.Wp) {
    int v[3] = {nm.pad[0], nm.pad[1], nm.pad[2]};
    if (inside) resized_pixel(src + im.src_offset, im.Hs, im.Ws, im.Hr, im.Wr, y, (flips >> n & 1u) ? im.Wr - 1 - x : x, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = normalise(v[c], nm.mean[c], nm.stdv[c]);
  }
  const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
  OutT* d = dst + (size_t)n * 3 * plane;
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c * plane + p] = from_f32<OutT>(o[c]);
  if (mask) mask[(size_t)n * plane + p] = from_f32<OutT>(inside ? 0.f : 1.f);
}

// one row of a tiles launch: the (Hs, Ws) window whose first byte is src + src_offset, inside an image `pitch` pixels wide
struct TileImage {
  int64_t src_offset;
  int pitch, Hs, Ws, Hr, Wr, Hp, Wp;
};
struct TileTable {
  TileImage img[kPreBatchMax];
};

// preprocess_batch_kernel with a crop per row: the row's source is a window of an uploaded image, resized as the
// contiguous copy of that window would be; rows may read windows of the same image.  (Its own body, as the views kernel's.)
template <class OutT>
__global__ __launch_bounds__(256) void preprocess_tiles_kernel(const unsigned char* __restrict__ src, TileTable tab,
                                                               BatchNorm nm, int H, int W, OutT* __restrict__ dst,
                                                               OutT* __restrict__ mask) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  const int n = blockIdx.z;
  if (x >= W) return;
  const TileImage im = tab.img[n];
  const bool inside = y < im.Hr && x < im.Wr;
  float o[3] = {nm.fill, nm.fill, nm.fill};
  if (y < im.Hp && x < im.Wp) {
    int v[3] = {nm.pad[0], nm.pad[1], nm.pad[2]};
    if (inside) resized_pixel(src + im.src_offset, im.Hs, im.Ws, im.pitch, im.Hr, im.Wr, y, x, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = normalise(v[c], nm.mean[c], nm.stdv[c]);
  }
  const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
  OutT* d = dst + (size_t)n * 3 * plane;
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c * plane + p] = from_f32<OutT>(o[c]);
  if (mask) mask[(size_t)n * plane + p] = from_f32<OutT>(inside ? 0.f : 1.f);
}

// torchvision nms's suppression test of candidate j by kept box i (area ia), fp32: IoU > thr
__device__ __forceinline__ bool iou_above(float ix1, float iy1, float ix2, float iy2, float ia, float jx1, float jy1,
                                          float jx2, float jy2, float thr) {
  const float w = fmaxf(0.f, fminf(ix2, jx2) - fmaxf(ix1, jx1));
  const float h = fmaxf(0.f, fminf(iy2, jy2) - fmaxf(iy1, jy1));
  const float inter = w * h;
  const float iou = inter / (ia + (jx2 - jx1) * (jy2 - jy1) - inter);
  return iou > thr;
}

// one workgroup; boxes / labels in descending score order.  keep[i] = 1 if i survives.
__global__ __launch_bounds__(1024) void batched_nms_kernel(const float* __restrict__ boxes,
                                                           const int64_t* __restrict__ labels, int N, float thr,
                                                           unsigned char* __restrict__ keep) {
  extern __shared__ unsigned char s_keep[];
  for (int j = threadIdx.x; j < N; j += blockDim.x) s_keep[j] = 1;
  __syncthreads();
  for (int i = 0; i < N; ++i) {
    if (s_keep[i]) {  // uniform across the workgroup (read after the barrier below)
      const float ix1 = boxes[4 * i], iy1 = boxes[4 * i + 1], ix2 = boxes[4 * i + 2], iy2 = boxes[4 * i + 3];
      const float ia = (ix2 - ix1) * (iy2 - iy1);
      const int64_t il = labels[i];
      for (int j = i + 1 + threadIdx.x; j < N; j += blockDim.x) {
        if (!s_keep[j] || labels[j] != il) continue;
        if (iou_above(ix1, iy1, ix2, iy2, ia, boxes[4 * j], boxes[4 * j + 1], boxes[4 * j + 2], boxes[4 * j + 3], thr))
          s_keep[j] = 0;
      }
    }
    __syncthreads();
  }
  for (int j = threadIdx.x; j < N; j += blockDim.x) keep[j] = s_keep[j];
}

constexpr int kPostMaxQ = CODETR_POSTPROCESS_MAX_Q;  // detections per image: one per thread of the workgroup

// descending sort key of a score, the order of the radix sort behind torch.sort of fp32 keys on this platform: the
// order-preserving image of the bits, so a NaN with the sign bit clear sorts above +inf and one with it set below -inf
// (the bf16 / f16 NaN of a model is the former); -0 is taken as +0
__device__ __forceinline__ unsigned score_key(float s) {
  const unsigned u = __float_as_uint(s == 0.f ? 0.f : s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// grid N, 1024 threads: image n's Q detections -> its kept detections, compacted in output order, count[n] of them.
// Rows [count, Q) of the outputs are zero.
template <class T>
__global__ __launch_bounds__(1024) void postprocess_kernel(const T* __restrict__ boxes, const T* __restrict__ scores,
                                                           const int64_t* __restrict__ labels,
                                                           const T* __restrict__ divisors, int Q, int use_thr, float thr,
                                                           int use_nms, float iou_thr, T* __restrict__ boxes_out,
                                                           T* __restrict__ scores_out, int64_t* __restrict__ labels_out,
                                                           int* __restrict__ count) {
  __shared__ unsigned long long s_key[kPostMaxQ];  // score key << 32 | (2^32 - 1 - index); 0 = dropped
  __shared__ float4 s_box[kPostMaxQ];              // candidates in output order, fp32
  __shared__ int64_t s_lab[kPostMaxQ];
  __shared__ unsigned char s_keep[kPostMaxQ];
  __shared__ int s_wave[kPostMaxQ / 64];
  const int tid = threadIdx.x;
  const size_t n = blockIdx.x;
  const T* bx = boxes + n * Q * 4;
  const T* sc = scores + n * Q;
  const int64_t* lb = labels + n * Q;

  // 1. score threshold, compared at T's precision (`scores > thr` on a T tensor converts the scalar to T)
  const float thr_t = to_f32(from_f32<T>(thr));
  unsigned long long key = 0;
  if (tid < Q) {
    const float s = to_f32(sc[tid]);
    if (!use_thr || s > thr_t)
      key = ((unsigned long long)(use_nms ? score_key(s) : 1u) << 32) | (unsigned long long)(0xffffffffu - (unsigned)tid);
  }
  s_key[tid] = key;
  const int V = __syncthreads_count(key != 0ull);  // candidates; barrier: s_key complete

  // 2. bitonic sort of the 1024 keys, descending: ties (and, without NMS, everything) in ascending index order
  for (int size = 2; size <= kPostMaxQ; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < kPostMaxQ / 2) {
        const int lo = 2 * tid - (tid & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = s_key[lo], b = s_key[hi];
        if ((a < b) == desc) {
          s_key[lo] = b;
          s_key[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  const unsigned src = 0xffffffffu - (unsigned)s_key[tid];  // (meaningful for tid < V)
  if (tid < V) {
    s_box[tid] = make_float4(to_f32(bx[4 * src]), to_f32(bx[4 * src + 1]), to_f32(bx[4 * src + 2]),
                             to_f32(bx[4 * src + 3]));
    s_lab[tid] = lb[src];
    s_keep[tid] = 1;
  }
  __syncthreads();

  // 3. greedy per-class NMS over the candidates in score order (batched_nms_kernel's visiting order and arithmetic)
  if (use_nms) {
    for (int i = 0; i < V; ++i) {
      if (!s_keep[i]) continue;  // uniform: nothing was written since the last barrier
      const float4 bi = s_box[i];
      const float ia = (bi.z - bi.x) * (bi.w - bi.y);
      if (tid > i && tid < V && s_keep[tid] && s_lab[tid] == s_lab[i]) {
        const float4 bj = s_box[tid];
        if (iou_above(bi.x, bi.y, bi.z, bi.w, ia, bj.x, bj.y, bj.z, bj.w, iou_thr)) s_keep[tid] = 0;
      }
      __syncthreads();
    }
  }

  // 4. compaction (ballot + wave totals) and the rescale: fp32 divide, one rounding to T
  const bool kept = tid < V && s_keep[tid];
  const unsigned long long bal = __ballot(kept);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) s_wave[wave] = __popcll(bal);
  __syncthreads();
  int pos = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
  for (int w = 0; w < kPostMaxQ / 64; ++w) {
    const int c = s_wave[w];
    pos += w < wave ? c : 0;
    total += c;
  }
  T* bo = boxes_out + n * Q * 4;
  T* so = scores_out + n * Q;
  int64_t* lo = labels_out + n * Q;
  if (kept) {
    const T* dv = divisors + n * 4;
    const float4 b = s_box[tid];
    bo[4 * pos] = from_f32<T>(b.x / to_f32(dv[0]));
    bo[4 * pos + 1] = from_f32<T>(b.y / to_f32(dv[1]));
    bo[4 * pos + 2] = from_f32<T>(b.z / to_f32(dv[2]));
    bo[4 * pos + 3] = from_f32<T>(b.w / to_f32(dv[3]));
    so[pos] = sc[src];
    lo[pos] = s_lab[tid];
  }
  if (tid >= total && tid < Q) {  // (kept rows are < total)
    const T z = from_f32<T>(0.f);
    bo[4 * tid] = z;
    bo[4 * tid + 1] = z;
    bo[4 * tid + 2] = z;
    bo[4 * tid + 3] = z;
    so[tid] = z;
    lo[tid] = 0;
  }
  if (tid == 0) count[n] = total;
}

// ---- building blocks of the 1024-thread workgroups of postprocess_softnms_kernel and tta_merge_kernel: each of the two
// is its own front end followed by the same calls (postprocess_kernel above uses none of them: its machine code is pinned)
constexpr int kNmsThreads = 1024, kNmsWaves = kNmsThreads / 64;
static_assert(kPostMaxQ == kNmsThreads, "one candidate per thread");

// an index as the minor part of a descending key: the lower index sorts first.  Its own inverse.
__device__ __forceinline__ unsigned inv_index(unsigned idx) { return 0xffffffffu - idx; }
// THE tie rule: (score key, index) as one 64-bit key -- the higher score first, equal scores in ascending index order
__device__ __forceinline__ unsigned long long pack_key(unsigned key, unsigned idx) {
  return ((unsigned long long)key << 32) | (unsigned long long)inv_index(idx);
}
__device__ __forceinline__ unsigned long long pack_key(float score, unsigned idx) { return pack_key(score_key(score), idx); }

// the key layouts of the bitonic sort: order(lo, hi, desc) swaps slots lo < hi unless the larger (desc) / smaller one is in lo
struct ScoreKeys {  // one 64-bit key per slot
  unsigned long long* key;
  __device__ __forceinline__ void order(int lo, int hi, bool desc) const {
    const unsigned long long a = key[lo], b = key[hi];
    if ((a < b) == desc) {
      key[lo] = b;
      key[hi] = a;
    }
  }
};
struct LabelIndexKeys {  // (label bits, inverted index) per slot, the empty slots (0, 0); equal pairs do not swap
  unsigned long long* lab;
  unsigned* idx;
  __device__ __forceinline__ void order(int lo, int hi, bool desc) const {
    const unsigned long long al = lab[lo], bl = lab[hi];
    const unsigned ai = idx[lo], bi = idx[hi];
    const bool less = al < bl || (al == bl && ai < bi);
    if (less == desc && (al != bl || ai != bi)) {
      lab[lo] = bl;
      lab[hi] = al;
      idx[lo] = bi;
      idx[hi] = ai;
    }
  }
};

// in-place descending bitonic sort of P (a power of two <= kMaxP) LDS slots; a thread takes pairs tid, tid + 1024, ... of a
// step, which is one pair and no loop for kMaxP <= 2048.  Ends with a barrier (for P >= 2).
template <int kMaxP, class Keys>
__device__ __forceinline__ void bitonic_desc(Keys keys, int P, int tid) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int t = tid; t < kMaxP / 2; t += kNmsThreads) {
        if (t < P / 2) {
          const int lo = 2 * t - (t & (stride - 1));
          keys.order(lo, lo + stride, (lo & size) == 0);
        }
      }
      __syncthreads();
    }
  }
}

// exclusive scan of a predicate over the workgroup (ballot + wave totals) -> the number of set predicates in the threads
// before this one, `total` = in all of them.  One barrier after s_wave is written: the caller sees to it that s_wave is free.
__device__ __forceinline__ int block_scan(bool pred, int* s_wave, int lane, int wave, int& total) {
  const unsigned long long bal = __ballot(pred);
  if (lane == 0) s_wave[wave] = __popcll(bal);
  __syncthreads();
  int pos = __popcll(bal & ((1ull << lane) - 1ull));
  total = 0;
#pragma unroll
  for (int w = 0; w < kNmsWaves; ++w) {
    const int c = s_wave[w];
    pos += w < wave ? c : 0;
    total += c;
  }
  return pos;
}

// sum of one int per thread over the workgroup, for the kernel with several slots per thread (a 0 / 1 per thread is
// __syncthreads_count).  Two barriers: s_wave may be in use before, everything written before is visible after.
__device__ __forceinline__ int block_sum(int v, int* s_wave, int lane, int wave) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if (lane == 0) s_wave[wave] = v;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < kNmsWaves; ++w) total += s_wave[w];
  return total;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}

// maximum of one key per thread over the workgroup (one barrier)
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* s_wmax, int lane,
                                                            int wave) {
  v = wave_max_u64(v);
  if (lane == 0) s_wmax[wave] = v;
  __syncthreads();
  unsigned long long g = 0;
#pragma unroll
  for (int w = 0; w < kNmsWaves; ++w) g = s_wmax[w] > g ? s_wmax[w] : g;
  return g;
}

// output row r of an image: the box rounded once to T (a rescale is the caller's: IEEE divide before the call)
template <class T>
__device__ __forceinline__ void write_row(T* bo, T* so, int64_t* lo, int* io, int r, float4 box, T score, int64_t label,
                                          int index) {
  bo[4 * r] = from_f32<T>(box.x);
  bo[4 * r + 1] = from_f32<T>(box.y);
  bo[4 * r + 2] = from_f32<T>(box.z);
  bo[4 * r + 3] = from_f32<T>(box.w);
  so[r] = score;
  lo[r] = label;
  io[r] = index;
}
template <class T>
__device__ __forceinline__ void zero_row(T* bo, T* so, int64_t* lo, int* io, int r) {
  write_row(bo, so, lo, io, r, make_float4(0.f, 0.f, 0.f, 0.f), from_f32<T>(0.f), 0, 0);
}

// ---- per-class greedy NMS over label segments: soft-NMS and the merge of test-time augmentation's views
// (include/codetr_hip.h states the semantics of both) ----------------------------------------------------------------------

// The IoU of the picked box k and candidate j is box_prims.h's box_iou over box_area: an area may be stored or computed
// again (run_segments' kStoredArea, the one policy difference of the two kernels).
// intersection over the smaller area (SAHI's IOS), the same rounded intersection; NaN when the smaller area is 0
__device__ __forceinline__ float ios_overlap(float4 bk, float ak, float4 bj, float aj) {
#pragma clang fp contract(off)
  const float w = fmaxf(0.f, fminf(bk.z, bj.z) - fmaxf(bk.x, bj.x));
  const float h = fmaxf(0.f, fminf(bk.w, bj.w) - fmaxf(bk.y, bj.y));
  const float inter = w * h;
  return inter / fminf(ak, aj);
}
// the box around two boxes: min and max only, so exact and free of the order the boxes come in
__device__ __forceinline__ float4 box_union(float4 a, float4 b) {
  return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}
__device__ __forceinline__ float4 wave_box_union(float4 v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1)
    v = box_union(v, make_float4(__shfl_xor(v.x, m, 64), __shfl_xor(v.y, m, 64), __shfl_xor(v.z, m, 64), __shfl_xor(v.w, m, 64)));
  return v;
}

// after the (label, index) sort of V live candidates: s_seg[0 .. S) = the first position of every label segment,
// s_seg[S] = V -> S.  kMaxP / 1024 positions per thread, a round each; with one round s_wave must be free at the call.
// Ends with a barrier.
template <int kMaxP>
__device__ __forceinline__ int segment_starts(const unsigned long long* s_lab, int V, unsigned short* s_seg, int* s_wave,
                                              int tid) {
  int S = 0;  // (uniform)
  for (int base = 0; base < kMaxP && (base == 0 || base < V); base += kNmsThreads) {
    const int p = base + tid;
    const bool head = p < V && (p == 0 || s_lab[p] != s_lab[p - 1]);
    if (kMaxP > kNmsThreads) __syncthreads();  // s_wave is free (the reads of the previous round, or of a block_sum, are done)
    int heads;
    const int hpos = S + block_scan(head, s_wave, tid & 63, tid >> 6, heads);
    if (head) s_seg[hpos] = (unsigned short)p;
    S += heads;
  }
  if (tid == 0) s_seg[S] = (unsigned short)V;
  __syncthreads();
  return S;
}

// the greedy chains: a wave takes whole segments; lane l holds positions a + l + 64 e (bit e of `alive`: Mask has a bit for
// every position of a lane -- unsigned for segments of up to 1024, unsigned long long up to 4096).  The pick is a wave
// reduction of pack_key(current score, position): highest score, ties to the lowest position = the lowest index.  It is
// emitted into s_out under its index with the score it has now, then decides over the others of its segment:
//   hard (only where kHardToo)  overlap > iou_thr: gone                       (a NaN overlap compares false: kept)
//   soft                        overlap >= iou_thr: score * (1 - overlap), or * 0 unless `linear`; score < min_score: gone
// kStoredArea: the areas are read from s_area (next to s_score in LDS, so that one instruction reads both), else
// computed again (s_area unused).  No workgroup barrier in here: a position's score is read and written by its own lane only.
// kSlice (the slice merge, hard only) adds two switches: `ios` measures the overlap as intersection over the smaller area,
// and `nmm` (non-maximum merging) has the pick absorb what it retires -- every lane gathers the box around its retired
// positions, a wave reduction joins them with k's and the owner stores the result in s_box[k], which no later round reads
// (k is retired; every overlap of this round was measured against the bk read before).
template <class Mask, bool kHardToo, bool kStoredArea, bool kSlice = false>
__device__ __forceinline__ void run_segments(const unsigned short* s_seg, int S, float4* s_box, const float* s_area,
                                             float* s_score, const unsigned* s_idx, unsigned long long* s_out, bool hard,
                                             bool linear, float iou_thr, float min_score, int lane, int wave,
                                             bool ios = false, bool nmm = false) {
  constexpr Mask kOne = 1;
  for (int seg = wave; seg < S; seg += kNmsWaves) {
    const int a = s_seg[seg], b = s_seg[seg + 1];
    const int ne = (b - a + 63) >> 6;  // <= the bits of Mask
    Mask alive = 0;
    for (int e = 0; e < ne; ++e) alive |= (a + lane + 64 * e < b) ? kOne << e : Mask(0);
    for (;;) {
      unsigned long long best = 0;
      for (int e = 0; e < ne; ++e) {
        if (alive >> e & kOne) {
          const int p = a + lane + 64 * e;
          const unsigned long long k = pack_key(s_score[p], (unsigned)p);
          best = k > best ? k : best;
        }
      }
      best = wave_max_u64(best);
      if (best == 0ull) break;  // (wave-uniform) the segment is exhausted
      const int k = (int)inv_index((unsigned)best);
      if (((k - a) & 63) == lane) {  // the owner emits k with its current score and retires it
        alive &= ~(kOne << ((k - a) >> 6));
        s_out[k] = (best & 0xffffffff00000000ull) | s_idx[k];  // (s_idx holds the minor key, inv_index(index), already)
      }
      const float4 bk = s_box[k];
      const float ak = kStoredArea ? s_area[k] : box_area(bk);
      float4 grown = bk;  // (kSlice && nmm) k and what this lane's positions gave up to it
      for (int e = 0; e < ne; ++e) {
        if (alive >> e & kOne) {
          const int p = a + lane + 64 * e;
          const float4 bj = s_box[p];
          const float aj = kStoredArea ? s_area[p] : box_area(bj);
          const float ovr = (kSlice && ios) ? ios_overlap(bk, ak, bj, aj) : box_iou(bk, ak, bj, aj);
          if (kHardToo && hard) {
            if (ovr > iou_thr) {
              alive &= ~(kOne << e);
              if (kSlice && nmm) grown = box_union(grown, bj);
            }
          } else {
            float sj = s_score[p];
            if (ovr >= iou_thr) {  // (a NaN overlap compares false: weight 1)
              sj = sj * (linear ? 1.f - ovr : 0.f);
              s_score[p] = sj;
            }
            if (sj < min_score) alive &= ~(kOne << e);
          }
        }
      }
      if (kSlice && nmm) {
        grown = wave_box_union(grown);
        if (((k - a) & 63) == lane) s_box[k] = grown;
      }
    }
  }
}

// grid N, 1024 threads: image n's Q candidates -> its soft-NMS detections in output order (decayed score descending,
// ties by ascending query index), cut to max_keep, count[n] of them.  Rows [count, Q) of the outputs are zero.
template <class T>
__global__ __launch_bounds__(kNmsThreads) void postprocess_softnms_kernel(
    const T* __restrict__ boxes, const T* __restrict__ scores, const int64_t* __restrict__ labels,
    const T* __restrict__ divisors, int Q, int use_thr, float thr, int linear, float iou_thr, float min_score,
    int max_keep, T* __restrict__ boxes_out, T* __restrict__ scores_out, int64_t* __restrict__ labels_out,
    int* __restrict__ index_out, int* __restrict__ count) {
  __shared__ unsigned long long s_lab[kPostMaxQ];  // sort 1, major key: the label's bits (live candidates)
  __shared__ unsigned s_idx[kPostMaxQ];            // sort 1, minor key: inv_index(query index); 0 = dropped
  __shared__ unsigned long long s_out[kPostMaxQ];  // emitted: pack_key(decayed score, query index); else 0
  __shared__ float4 s_box[kPostMaxQ];              // by position after sort 1 (label segments, ascending query index)
  __shared__ float s_area[kPostMaxQ];              // (stored here, computed again in the merge, whose LDS has no room)
  __shared__ float s_score[kPostMaxQ];             // current (decaying) score; touched by the position's own lane only
  __shared__ unsigned short s_seg[kPostMaxQ + 1];  // first position of every label segment, then V
  __shared__ unsigned short s_pos[kPostMaxQ];      // query index -> position
  __shared__ unsigned long long s_wmax[kNmsWaves];
  __shared__ int s_wave[kNmsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = blockIdx.x;
  const T* bx = boxes + n * Q * 4;
  const T* sc = scores + n * Q;
  const int64_t* lb = labels + n * Q;
  int P = 1;  // the sorts run over the next power of two >= Q
  while (P < Q) P <<= 1;

  // front end: score threshold at T's precision (as postprocess_kernel), the global maximum g (ties: lowest index), then
  // everything below min_score goes, except g (mmcv emits its first pick unchecked)
  const float thr_t = to_f32(from_f32<T>(thr));
  unsigned long long key = 0;
  float s = 0.f;
  if (tid < Q) {
    s = to_f32(sc[tid]);
    if (!use_thr || s > thr_t) key = pack_key(s, (unsigned)tid);
  }
  const unsigned long long g = block_max_u64(key, s_wmax, lane, wave);
  const bool live = key != 0ull && (key == g || !(s < min_score));
  s_lab[tid] = live ? (unsigned long long)lb[tid] : 0ull;
  s_idx[tid] = live ? inv_index((unsigned)tid) : 0u;
  s_out[tid] = 0ull;
  const int V = __syncthreads_count(live);  // barrier: the sort keys are complete

  // 1. by (label, index), descending: every label a contiguous segment in ascending index order, the dropped slots last
  bitonic_desc<kPostMaxQ>(LabelIndexKeys{s_lab, s_idx}, P, tid);
  if (tid < V) {
    const unsigned src = inv_index(s_idx[tid]);
    const float4 b = make_float4(to_f32(bx[4 * src]), to_f32(bx[4 * src + 1]), to_f32(bx[4 * src + 2]),
                                 to_f32(bx[4 * src + 3]));
    s_box[tid] = b;
    s_area[tid] = box_area(b);
    s_score[tid] = to_f32(sc[src]);
    s_pos[src] = (unsigned short)tid;
  }
  // 2. - 4. segments, chains (up to 16 positions per lane), the emitted detections by (decayed score, index)
  const int S = segment_starts<kPostMaxQ>(s_lab, V, s_seg, s_wave, tid);
  run_segments<unsigned, false, true>(s_seg, S, s_box, s_area, s_score, s_idx, s_out, false, linear != 0, iou_thr, min_score, lane,
                                      wave);
  __syncthreads();
  bitonic_desc<kPostMaxQ>(ScoreKeys{s_out}, P, tid);
  const unsigned long long okey = s_out[tid];
  const int E = __syncthreads_count(okey != 0ull);
  const int M = (max_keep > 0 && max_keep < E) ? max_keep : E;

  // 5. cut, rescale: fp32 divide, one rounding to T
  T* bo = boxes_out + n * Q * 4;
  T* so = scores_out + n * Q;
  int64_t* lo = labels_out + n * Q;
  int* io = index_out + n * Q;
  if (tid < M) {
    const unsigned src = inv_index((unsigned)okey);
    const int p = s_pos[src];
    const T* dv = divisors + n * 4;
    const float4 b = s_box[p];
    write_row(bo, so, lo, io, tid,
              make_float4(b.x / to_f32(dv[0]), b.y / to_f32(dv[1]), b.z / to_f32(dv[2]), b.w / to_f32(dv[3])),
              from_f32<T>(s_score[p]), lb[src], (int)src);
  } else if (tid < Q) {
    zero_row(bo, so, lo, io, tid);
  }
  if (tid == 0) count[n] = M;
}

constexpr int kTtaMaxC = CODETR_TTA_MAX_CANDIDATES;  // V * Q of a merge: positions 0 .. 4095 fit the 16-bit tables

// dynamic LDS of tta_merge_kernel over P slots: box 16, label / output key 8, score 4, index 4, position 2, segment 2
// bytes per slot = 36 P + 16; 144 KB at P = 4096, hence the opt-in of large_lds.h
constexpr size_t tta_lds_bytes(int P) { return (size_t)P * 36 + 16; }

// grid N, 1024 threads: image n's V views of Q detections (rows j < count[v, n] are candidates, c = v Q + j) -> the merged
// detections in output order, cut to max_keep, count_out[n] of them; rows [count_out, K) of the outputs are zero.
// P = the power of two >= V Q.  mode: CODETR_TTA_NMS_*.
template <class T>
__global__ __launch_bounds__(kNmsThreads) void tta_merge_kernel(
    const T* __restrict__ boxes, const T* __restrict__ scores, const int64_t* __restrict__ labels,
    const int* __restrict__ count, int V, int N, int Q, int P, unsigned flip_mask, const float* __restrict__ width,
    int mode, float iou_thr, float min_score, int max_keep, int K, T* __restrict__ boxes_out,
    T* __restrict__ scores_out, int64_t* __restrict__ labels_out, int* __restrict__ index_out,
    int* __restrict__ count_out) {
  extern __shared__ __align__(16) unsigned char tta_lds[];
  float4* s_box = reinterpret_cast<float4*>(tta_lds);  // by position after sort 1 (label segments, ascending c)
  unsigned long long* s_lab = reinterpret_cast<unsigned long long*>(tta_lds + (size_t)16 * P);  // sort 1, major key
  unsigned long long* s_out = s_lab;  // (after the segments are found) emitted: pack_key(score, c); else 0
  float* s_score = reinterpret_cast<float*>(tta_lds + (size_t)24 * P);  // current score; its own lane's only
  unsigned* s_idx = reinterpret_cast<unsigned*>(tta_lds + (size_t)28 * P);  // sort 1, minor key: inv_index(c); 0 = none
  unsigned short* s_pos = reinterpret_cast<unsigned short*>(tta_lds + (size_t)32 * P);  // c -> position
  unsigned short* s_seg = reinterpret_cast<unsigned short*>(tta_lds + (size_t)34 * P);  // segment starts, then Vn
  __shared__ unsigned long long s_wmax[kNmsWaves];
  __shared__ int s_wave[kNmsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  const int C = V * Q;
  const bool soft = mode != CODETR_TTA_NMS_HARD;
  // element (v, n, j) of the stacked inputs
  auto at = [&](int c, int& v) -> size_t {
    v = c / Q;
    return ((size_t)v * N + n) * Q + (size_t)(c - v * Q);
  };

  // front end: (soft modes) the global maximum g (ties: lowest c), which the min_score drop spares; then the sort keys of
  // the live candidates, (label, c), everything else 0
  unsigned long long g = 0;
  if (soft) {
    unsigned long long best = 0;
    for (int c = tid; c < C; c += kNmsThreads) {
      int v;
      const size_t e = at(c, v);
      if (c - v * Q < count[v * N + n]) {
        const unsigned long long k = pack_key(to_f32(scores[e]), (unsigned)c);
        best = k > best ? k : best;
      }
    }
    g = block_max_u64(best, s_wmax, lane, wave);
  }
  int nlive = 0;
  for (int c = tid; c < P; c += kNmsThreads) {
    bool live = false;
    unsigned long long lab = 0;
    if (c < C) {
      int v;
      const size_t e = at(c, v);
      if (c - v * Q < count[v * N + n]) {
        const float s = to_f32(scores[e]);
        live = !soft || pack_key(s, (unsigned)c) == g || !(s < min_score);
        lab = (unsigned long long)labels[e];
      }
    }
    s_lab[c] = live ? lab : 0ull;
    s_idx[c] = live ? inv_index((unsigned)c) : 0u;
    nlive += live ? 1 : 0;
  }
  const int Vn = block_sum(nlive, s_wave, lane, wave);  // (its barriers: the sort keys are complete)

  // 1. by (label, c), descending: every label a contiguous segment in ascending c, empty slots last; boxes un-flipped
  bitonic_desc<kTtaMaxC>(LabelIndexKeys{s_lab, s_idx}, P, tid);
  const float Wimg = width[n];
  for (int p = tid; p < Vn; p += kNmsThreads) {
    const unsigned c = inv_index(s_idx[p]);
    int v;
    const size_t e = at((int)c, v);
    float4 b = make_float4(to_f32(boxes[4 * e]), to_f32(boxes[4 * e + 1]), to_f32(boxes[4 * e + 2]), to_f32(boxes[4 * e + 3]));
    if (flip_mask >> v & 1u) {  // un-flip: (W - x2, y1, W - x1, y2)
      const float x1 = Wimg - b.z, x2 = Wimg - b.x;
      b.x = x1;
      b.z = x2;
    }
    s_box[p] = b;
    s_score[p] = to_f32(scores[e]);
    s_pos[c] = (unsigned short)p;
  }
  // 2. - 4. segments (the labels were then read for the last time: their array becomes s_out), chains (up to 64 positions
  //    per lane), the emitted detections by (score, c)
  const int S = segment_starts<kTtaMaxC>(s_lab, Vn, s_seg, s_wave, tid);
  for (int p = tid; p < P; p += kNmsThreads) s_out[p] = 0ull;
  __syncthreads();
  run_segments<unsigned long long, true, false>(s_seg, S, s_box, nullptr, s_score, s_idx, s_out, !soft,
                                                mode == CODETR_TTA_NMS_SOFT_LINEAR, iou_thr, min_score, lane, wave);
  __syncthreads();
  bitonic_desc<kTtaMaxC>(ScoreKeys{s_out}, P, tid);
  int nout = 0;
  for (int p = tid; p < P; p += kNmsThreads) nout += s_out[p] != 0ull ? 1 : 0;
  const int E = block_sum(nout, s_wave, lane, wave);
  const int M = (max_keep > 0 && max_keep < E) ? max_keep : E;

  // 5. cut, round once to T
  T* bo = boxes_out + (size_t)n * K * 4;
  T* so = scores_out + (size_t)n * K;
  int64_t* lo = labels_out + (size_t)n * K;
  int* io = index_out + (size_t)n * K;
  for (int r = tid; r < K; r += kNmsThreads) {
    if (r < M) {
      const unsigned c = inv_index((unsigned)s_out[r]);
      const int p = s_pos[c];
      int v;
      write_row(bo, so, lo, io, r, s_box[p], from_f32<T>(s_score[p]), labels[at((int)c, v)], (int)c);
    } else {
      zero_row(bo, so, lo, io, r);
    }
  }
  if (tid == 0) count_out[n] = M;
}

constexpr int kSliceMaxV = CODETR_SLICE_MAX_VIEWS;

// grid N, 1024 threads: the detections of image n's V views (tile rows of the stacked [R, Q] inputs, rows[n, v]; a row
// outside [0, R) is an absent view; candidate c = v Q + j for j < count[row]) shifted by the row's origin and clipped to the
// image -> the fused detections in output order, cut to max_keep, count_out[n] of them; rows [count_out, K) are zero.
// tta_merge_kernel's LDS layout and steps with a front end of its own; P = the power of two >= V Q.
// metric: CODETR_SLICE_IOU / _IOS, mode: CODETR_SLICE_NMS / _NMM.
template <class T>
__global__ __launch_bounds__(kNmsThreads) void slice_merge_kernel(
    const T* __restrict__ boxes, const T* __restrict__ scores, const int64_t* __restrict__ labels,
    const int* __restrict__ count, const int* __restrict__ rows, const float* __restrict__ origin,
    const float* __restrict__ size, int R, int V, int Q, int P, int metric, int mode, float thr, int agnostic,
    int max_keep, int K, T* __restrict__ boxes_out, T* __restrict__ scores_out, int64_t* __restrict__ labels_out,
    int* __restrict__ index_out, int* __restrict__ count_out) {
  extern __shared__ __align__(16) unsigned char slice_lds[];
  float4* s_box = reinterpret_cast<float4*>(slice_lds);  // by position after sort 1; a pick's box becomes its union (NMM)
  unsigned long long* s_lab = reinterpret_cast<unsigned long long*>(slice_lds + (size_t)16 * P);  // sort 1, major key
  unsigned long long* s_out = s_lab;  // (after the segments are found) emitted: pack_key(score, c); else 0
  float* s_score = reinterpret_cast<float*>(slice_lds + (size_t)24 * P);
  unsigned* s_idx = reinterpret_cast<unsigned*>(slice_lds + (size_t)28 * P);  // sort 1, minor key: inv_index(c); 0 = none
  unsigned short* s_pos = reinterpret_cast<unsigned short*>(slice_lds + (size_t)32 * P);  // c -> position
  unsigned short* s_seg = reinterpret_cast<unsigned short*>(slice_lds + (size_t)34 * P);  // segment starts, then Vn
  __shared__ int s_row[kSliceMaxV];  // the row of view v, its candidates (0 for an absent view)
  __shared__ int s_cnt[kSliceMaxV];
  __shared__ int s_wave[kNmsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  const int C = V * Q;
  if (tid < V) {
    const int r = rows[(size_t)n * V + tid];
    const bool present = r >= 0 && r < R;
    s_row[tid] = present ? r : 0;
    s_cnt[tid] = present ? count[r] : 0;
  }
  __syncthreads();
  // element (row of view v, j) of the stacked inputs
  auto at = [&](int c) -> size_t {
    const int v = c / Q;
    return (size_t)s_row[v] * Q + (size_t)(c - v * Q);
  };

  // front end: the sort keys of the candidates, (label, c) -- or (0, c): one segment -- everything else 0
  int nlive = 0;
  for (int c = tid; c < P; c += kNmsThreads) {
    bool live = false;
    unsigned long long lab = 0;
    if (c < C) {
      const int v = c / Q;
      if (c - v * Q < s_cnt[v]) {
        live = true;
        lab = agnostic ? 0ull : (unsigned long long)labels[at(c)];
      }
    }
    s_lab[c] = lab;
    s_idx[c] = live ? inv_index((unsigned)c) : 0u;
    nlive += live ? 1 : 0;
  }
  const int Vn = block_sum(nlive, s_wave, lane, wave);  // (its barriers: the sort keys are complete)

  // 1. by (label, c), descending: every label a contiguous segment in ascending c, empty slots last; boxes moved to the
  //    image's coordinates and clipped to it (fmaxf first: a NaN coordinate becomes 0)
  bitonic_desc<kTtaMaxC>(LabelIndexKeys{s_lab, s_idx}, P, tid);
  const float Wimg = size[2 * n], Himg = size[2 * n + 1];
  for (int p = tid; p < Vn; p += kNmsThreads) {
    const unsigned c = inv_index(s_idx[p]);
    const size_t e = at((int)c);
    const int r = s_row[c / Q];
    const float x0 = origin[2 * r], y0 = origin[2 * r + 1];
    s_box[p] = make_float4(fminf(fmaxf(to_f32(boxes[4 * e]) + x0, 0.f), Wimg), fminf(fmaxf(to_f32(boxes[4 * e + 1]) + y0, 0.f), Himg),
                           fminf(fmaxf(to_f32(boxes[4 * e + 2]) + x0, 0.f), Wimg), fminf(fmaxf(to_f32(boxes[4 * e + 3]) + y0, 0.f), Himg));
    s_score[p] = to_f32(scores[e]);
    s_pos[c] = (unsigned short)p;
  }
  // 2. - 4. as tta_merge_kernel; up to 1024 slots a lane holds at most 16 positions of a segment: the 32-bit mask
  const int S = segment_starts<kTtaMaxC>(s_lab, Vn, s_seg, s_wave, tid);
  for (int p = tid; p < P; p += kNmsThreads) s_out[p] = 0ull;
  __syncthreads();
  const bool ios = metric == CODETR_SLICE_IOS, nmm = mode == CODETR_SLICE_NMM;
  if (P <= kNmsThreads)
    run_segments<unsigned, true, false, true>(s_seg, S, s_box, nullptr, s_score, s_idx, s_out, true, false, thr, 0.f, lane, wave,
                                              ios, nmm);
  else
    run_segments<unsigned long long, true, false, true>(s_seg, S, s_box, nullptr, s_score, s_idx, s_out, true, false, thr, 0.f,
                                                        lane, wave, ios, nmm);
  __syncthreads();
  bitonic_desc<kTtaMaxC>(ScoreKeys{s_out}, P, tid);
  int nout = 0;
  for (int p = tid; p < P; p += kNmsThreads) nout += s_out[p] != 0ull ? 1 : 0;
  const int E = block_sum(nout, s_wave, lane, wave);
  const int M = (max_keep > 0 && max_keep < E) ? max_keep : E;

  // 5. cut, round once to T
  T* bo = boxes_out + (size_t)n * K * 4;
  T* so = scores_out + (size_t)n * K;
  int64_t* lo = labels_out + (size_t)n * K;
  int* io = index_out + (size_t)n * K;
  for (int r = tid; r < K; r += kNmsThreads) {
    if (r < M) {
      const unsigned c = inv_index((unsigned)s_out[r]);
      const int p = s_pos[c];
      write_row(bo, so, lo, io, r, s_box[p], from_f32<T>(s_score[p]), labels[at((int)c)], (int)c);
    } else {
      zero_row(bo, so, lo, io, r);
    }
  }
  if (tid == 0) count_out[n] = M;
}

// ---- weighted boxes fusion (include/codetr_wbf.h states the rule): tta_merge_kernel's operands, LDS layout and sorts with a
// chain of its own ---------------------------------------------------------------------------------------------------------
static_assert(CODETR_WBF_MAX_CANDIDATES == kTtaMaxC, "the WBF kernel uses the TTA merge's LDS layout and 16-bit tables");

struct WbfWeights {  // the weight of every view, in the kernargs
  float w[CODETR_TTA_MAX_VIEWS];
};

// a cluster's output key: (score, founder c) as pack_key orders them, with the votes (<= 4096: 13 bits) below the index
constexpr int kWbfVoteBits = 13;
__device__ __forceinline__ unsigned long long wbf_out_key(float score, unsigned c, unsigned votes) {
  return ((unsigned long long)score_key(score) << 32) | ((unsigned long long)(kTtaMaxC - 1 - c) << kWbfVoteBits) | votes;
}
__device__ __forceinline__ int lowest_bit(unsigned m) { return __builtin_ctz(m); }
__device__ __forceinline__ int lowest_bit(unsigned long long m) { return __builtin_ctzll(m); }

// the fusion chains: a wave takes whole segments; lane l holds positions a + l + 64 e and two masks over them, `todo` (not
// yet processed) and `found` (founders of a cluster).  A cluster lives in its founder's slots, which only the founder's
// lane reads or writes once it is founded: s_box = the sums SX1, SY1, SX2, SY2, s_score = SC, s_out = (bits of top) << 32 | n.
// A step: the pick k is a wave reduction of pack_key(conf, position) over `todo`; every lane measures k against its
// clusters; a wave reduction of pack_key(ovr, founder position) over those with ovr > iou_thr names the winner (highest
// ovr, ties to the lowest position = the lowest founder c), whose lane adds k to the sums -- or k's lane founds a cluster.
// At the end of a segment every founder's slots become what the epilogue reads: s_box the fused box, s_score the score,
// s_out the output key.  The step loop is counted (a segment of b - a positions takes b - a steps).  No workgroup barrier.
template <class Mask>
__device__ __forceinline__ void wbf_segments(const unsigned short* s_seg, int S, float4* s_box, float* s_score,
                                             const unsigned* s_idx, unsigned long long* s_out, bool conf_max, float iou_thr,
                                             float wsum, float wmax, int lane, int wave) {
#pragma clang fp contract(off)
  constexpr Mask kOne = 1;
  for (int seg = wave; seg < S; seg += kNmsWaves) {
    const int a = s_seg[seg], b = s_seg[seg + 1];
    const int ne = (b - a + 63) >> 6;  // <= the bits of Mask
    Mask todo = 0, found = 0;
    for (int e = 0; e < ne; ++e) todo |= (a + lane + 64 * e < b) ? kOne << e : Mask(0);
    for (int step = a; step < b; ++step) {
      unsigned long long best = 0;
      for (Mask m = todo; m != 0; m &= m - 1) {
        const int p = a + lane + 64 * lowest_bit(m);
        const unsigned long long k = pack_key(s_score[p], (unsigned)p);
        best = k > best ? k : best;
      }
      best = wave_max_u64(best);
      if (best == 0ull) break;  // (wave-uniform) the segment is exhausted
      const int k = (int)inv_index((unsigned)best);
      const float4 bk = s_box[k];
      const float ak = box_area(bk), ck = s_score[k];
      unsigned long long win = 0;
      for (Mask m = found; m != 0; m &= m - 1) {
        const int p = a + lane + 64 * lowest_bit(m);
        const float4 sum = s_box[p];
        const float sc = s_score[p];
        const float4 f = make_float4(sum.x / sc, sum.y / sc, sum.z / sc, sum.w / sc);
        const float ovr = box_iou(f, box_area(f), bk, ak);
        if (ovr > iou_thr) {  // (a NaN overlap compares false)
          const unsigned long long key = pack_key(ovr, (unsigned)p);
          win = key > win ? key : win;
        }
      }
      win = wave_max_u64(win);
      const bool mine = ((k - a) & 63) == lane;
      if (mine) todo &= ~(kOne << ((k - a) >> 6));
      if (win == 0ull) {  // (wave-uniform) k founds a cluster, in its own slots: s_score[k] is SC already
        if (mine) {
          found |= kOne << ((k - a) >> 6);
          s_box[k] = make_float4(ck * bk.x, ck * bk.y, ck * bk.z, ck * bk.w);
          s_out[k] = ((unsigned long long)__float_as_uint(ck) << 32) | 1ull;
        }
      } else {
        const int q = (int)inv_index((unsigned)win);
        if (((q - a) & 63) == lane) {
          float4 sum = s_box[q];
          const float px = ck * bk.x, py = ck * bk.y, pz = ck * bk.z, pw = ck * bk.w;
          sum.x = sum.x + px;
          sum.y = sum.y + py;
          sum.z = sum.z + pz;
          sum.w = sum.w + pw;
          s_box[q] = sum;
          s_score[q] = s_score[q] + ck;
          s_out[q] += 1ull;
        }
      }
    }
    for (Mask m = found; m != 0; m &= m - 1) {
      const int p = a + lane + 64 * lowest_bit(m);
      const float4 sum = s_box[p];
      const float sc = s_score[p];
      const unsigned long long st = s_out[p];
      const unsigned votes = (unsigned)st;
      const float nf = (float)votes, top = __uint_as_float((unsigned)(st >> 32));
      const float score = conf_max ? top / wmax : ((sc / nf) * fminf(nf, wsum)) / wsum;
      s_box[p] = make_float4(sum.x / sc, sum.y / sc, sum.z / sc, sum.w / sc);
      s_score[p] = score;
      s_out[p] = wbf_out_key(score, inv_index(s_idx[p]), votes);
    }
  }
}

// grid N, 1024 threads: image n's V views of Q detections (rows j < count[v, n] are candidates, c = v Q + j) -> the fused
// clusters in output order, cut to max_keep, count_out[n] of them; rows [count_out, K) of the outputs are zero.
// P = the power of two >= V Q; wsum, wmax: the sum (in view order) and the maximum of the V weights.
template <class T>
__global__ __launch_bounds__(kNmsThreads) void wbf_merge_kernel(
    const T* __restrict__ boxes, const T* __restrict__ scores, const int64_t* __restrict__ labels,
    const int* __restrict__ count, int V, int N, int Q, int P, unsigned flip_mask, const float* __restrict__ width,
    WbfWeights weights, float wsum, float wmax, int conf_max, float iou_thr, float skip_thr, int max_keep, int K,
    T* __restrict__ boxes_out, T* __restrict__ scores_out, int64_t* __restrict__ labels_out, int* __restrict__ index_out,
    int* __restrict__ count_out, int* __restrict__ votes_out) {
  extern __shared__ __align__(16) unsigned char wbf_lds[];
  float4* s_box = reinterpret_cast<float4*>(wbf_lds);  // by position after sort 1; a founder's: the sums, then the fused box
  unsigned long long* s_lab = reinterpret_cast<unsigned long long*>(wbf_lds + (size_t)16 * P);  // sort 1, major key
  unsigned long long* s_out = s_lab;  // (after the segments are found) a founder's (top, n), then its output key; else 0
  float* s_score = reinterpret_cast<float*>(wbf_lds + (size_t)24 * P);  // conf; a founder's: SC, then the score
  unsigned* s_idx = reinterpret_cast<unsigned*>(wbf_lds + (size_t)28 * P);  // sort 1, minor key: inv_index(c); 0 = none
  unsigned short* s_pos = reinterpret_cast<unsigned short*>(wbf_lds + (size_t)32 * P);  // c -> position
  unsigned short* s_seg = reinterpret_cast<unsigned short*>(wbf_lds + (size_t)34 * P);  // segment starts, then Vn
  __shared__ float s_w[CODETR_TTA_MAX_VIEWS];
  __shared__ int s_wave[kNmsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  const int C = V * Q;
  // element (v, n, j) of the stacked inputs
  auto at = [&](int c, int& v) -> size_t {
    v = c / Q;
    return ((size_t)v * N + n) * Q + (size_t)(c - v * Q);
  };
  if (tid < CODETR_TTA_MAX_VIEWS) {
    float w = 0.f;
#pragma unroll
    for (int v = 0; v < CODETR_TTA_MAX_VIEWS; ++v) w = tid == v ? weights.w[v] : w;  // (constant indices: no scratch copy)
    s_w[tid] = w;
  }
  __syncthreads();

  // front end: the sort keys of the live candidates, (label, c), everything else 0
  int nlive = 0;
  for (int c = tid; c < P; c += kNmsThreads) {
    bool live = false;
    unsigned long long lab = 0;
    if (c < C) {
      int v;
      const size_t e = at(c, v);
      if (c - v * Q < count[v * N + n]) {
        const float s = to_f32(scores[e]);
        const float conf = s * s_w[v];
        live = s >= skip_thr && conf > 0.f;  // (a NaN fails both)
        lab = (unsigned long long)labels[e];
      }
    }
    s_lab[c] = live ? lab : 0ull;
    s_idx[c] = live ? inv_index((unsigned)c) : 0u;
    nlive += live ? 1 : 0;
  }
  const int Vn = block_sum(nlive, s_wave, lane, wave);  // (its barriers: the sort keys are complete)

  // 1. by (label, c), descending: every label a contiguous segment in ascending c, empty slots last; boxes un-flipped
  bitonic_desc<kTtaMaxC>(LabelIndexKeys{s_lab, s_idx}, P, tid);
  const float Wimg = width[n];
  for (int p = tid; p < Vn; p += kNmsThreads) {
    const unsigned c = inv_index(s_idx[p]);
    int v;
    const size_t e = at((int)c, v);
    float4 b = make_float4(to_f32(boxes[4 * e]), to_f32(boxes[4 * e + 1]), to_f32(boxes[4 * e + 2]), to_f32(boxes[4 * e + 3]));
    if (flip_mask >> v & 1u) {  // un-flip: (W - x2, y1, W - x1, y2)
      const float x1 = Wimg - b.z, x2 = Wimg - b.x;
      b.x = x1;
      b.z = x2;
    }
    s_box[p] = b;
    s_score[p] = to_f32(scores[e]) * s_w[v];
    s_pos[c] = (unsigned short)p;
  }
  // 2. - 4. segments (the labels were then read for the last time: their array becomes s_out), the fusion chains (up to
  //    1024 slots a lane holds at most 16 positions of a segment: the 32-bit masks), the clusters by (score, founder c)
  const int S = segment_starts<kTtaMaxC>(s_lab, Vn, s_seg, s_wave, tid);
  for (int p = tid; p < P; p += kNmsThreads) s_out[p] = 0ull;
  __syncthreads();
  if (P <= kNmsThreads)
    wbf_segments<unsigned>(s_seg, S, s_box, s_score, s_idx, s_out, conf_max != 0, iou_thr, wsum, wmax, lane, wave);
  else
    wbf_segments<unsigned long long>(s_seg, S, s_box, s_score, s_idx, s_out, conf_max != 0, iou_thr, wsum, wmax, lane, wave);
  __syncthreads();
  bitonic_desc<kTtaMaxC>(ScoreKeys{s_out}, P, tid);
  int nout = 0;
  for (int p = tid; p < P; p += kNmsThreads) nout += s_out[p] != 0ull ? 1 : 0;
  const int E = block_sum(nout, s_wave, lane, wave);
  const int M = (max_keep > 0 && max_keep < E) ? max_keep : E;

  // 5. cut, round once to T
  T* bo = boxes_out + (size_t)n * K * 4;
  T* so = scores_out + (size_t)n * K;
  int64_t* lo = labels_out + (size_t)n * K;
  int* io = index_out + (size_t)n * K;
  int* vo = votes_out + (size_t)n * K;
  for (int r = tid; r < K; r += kNmsThreads) {
    if (r < M) {
      const unsigned low = (unsigned)s_out[r];
      const unsigned c = (unsigned)(kTtaMaxC - 1) - (low >> kWbfVoteBits);
      const int p = s_pos[c];
      int v;
      write_row(bo, so, lo, io, r, s_box[p], from_f32<T>(s_score[p]), labels[at((int)c, v)], (int)c);
      vo[r] = (int)(low & ((1u << kWbfVoteBits) - 1u));
    } else {
      zero_row(bo, so, lo, io, r);
      vo[r] = 0;
    }
  }
  if (tid == 0) count_out[n] = M;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// what a launch returns: 0, or the HIP error it left
int launched() {
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

template <class OutT>
int launch_pre(void* stream, const void* src, int64_t Hs, int64_t Ws, int64_t Hr, int64_t Wr, int64_t Hp, int64_t Wp,
               const float* mean, const float* stdv, const int* pad, void* dst, void* mask) {
  if (!src || !dst || !mean || !stdv || !pad || Hs <= 0 || Ws <= 0 || Hr <= 0 || Wr <= 0 || Hp < Hr || Wp < Wr)
    return CODETR_E_BADARG;
  if (Hs > 32767 || Ws > 32767 || Hp > 65535 || Wp > 0x7fffffffLL) return CODETR_E_TOO_LARGE;  // 2048 * 255 * 2048 fits int64; indices int
  for (int c = 0; c < 3; ++c)
    if (stdv[c] == 0.f || pad[c] < 0 || pad[c] > 255) return CODETR_E_BADARG;
  hipLaunchKernelGGL((preprocess_kernel<OutT>), dim3((unsigned)((Wp + 255) / 256), (unsigned)Hp), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned char*>(src), (int)Hs, (int)Ws, (int)Hr,
                     (int)Wr, (int)Hp, (int)Wp, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2], pad[0], pad[1],
                     pad[2], static_cast<OutT*>(dst), static_cast<OutT*>(mask));
  return launched();
}

// the normalisation of a batched preprocess call, checked
int pre_norm_args(const float* mean, const float* stdv, const int* pad, float pad_fill, BatchNorm& nm) {
  for (int c = 0; c < 3; ++c) {
    if (stdv[c] == 0.f || pad[c] < 0 || pad[c] > 255) return CODETR_E_BADARG;
    nm.mean[c] = mean[c];
    nm.stdv[c] = stdv[c];
    nm.pad[c] = pad[c];
  }
  nm.fill = pad_fill;
  return 0;
}

// the checks of a batched preprocess call and its kernel arguments; `cols` = 7 (codetr_preprocess_batch_u8_*) or 8
// (codetr_preprocess_views_u8_*: the eighth value of a row is its flip, gathered into `flips`)
int pre_batch_args(const void* src, int64_t src_bytes, int64_t N, const int64_t* images, int cols, int64_t H, int64_t W,
                   const float* mean, const float* stdv, const int* pad, float pad_fill, const void* dst, BatchTable& tab,
                   BatchNorm& nm, unsigned& flips) {
  if (!src || !images || !mean || !stdv || !pad || !dst || src_bytes <= 0 || N <= 0 || H <= 0 || W <= 0)
    return CODETR_E_BADARG;
  if (N > kPreBatchMax || H > 65535 || W > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (const int rc = pre_norm_args(mean, stdv, pad, pad_fill, nm)) return rc;
  flips = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = images + cols * n;  // src_offset, H_src, W_src, H_resized, W_resized, H_pad, W_pad[, flip]
    const int64_t off = r[0], Hs = r[1], Ws = r[2], Hr = r[3], Wr = r[4], Hp = r[5], Wp = r[6];
    if (off < 0 || Hs <= 0 || Ws <= 0 || Hr <= 0 || Wr <= 0 || Hp < Hr || Wp < Wr || Hp > H || Wp > W)
      return CODETR_E_BADARG;
    if (cols == 8 && r[7] != 0 && r[7] != 1) return CODETR_E_BADARG;
    if (Hs > 32767 || Ws > 32767) return CODETR_E_TOO_LARGE;
    if (off > src_bytes || Hs * Ws * 3 > src_bytes - off) return CODETR_E_BADARG;  // the image must lie in the buffer
    tab.img[n] = BatchImage{off, (int)Hs, (int)Ws, (int)Hr, (int)Wr, (int)Hp, (int)Wp};
    if (cols == 8 && r[7] == 1) flips |= 1u << n;
  }
  return 0;
}

// cols = 7: preprocess_batch_kernel; 8: preprocess_views_kernel
template <class OutT>
int launch_pre_rows(int cols, void* stream, const void* src, int64_t src_bytes, int64_t N, const int64_t* images, int64_t H,
                    int64_t W, const float* mean, const float* stdv, const int* pad, float pad_fill, void* dst,
                    void* mask) {
  BatchTable tab = {};
  BatchNorm nm;
  unsigned flips;
  if (const int rc = pre_batch_args(src, src_bytes, N, images, cols, H, W, mean, stdv, pad, pad_fill, dst, tab, nm, flips))
    return rc;
  const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)N);
  const auto s = static_cast<hipStream_t>(stream);
  const auto in = static_cast<const unsigned char*>(src);
  if (cols == 8)
    hipLaunchKernelGGL((preprocess_views_kernel<OutT>), grid, dim3(256), 0, s, in, tab, flips, nm, (int)H, (int)W,
                       static_cast<OutT*>(dst), static_cast<OutT*>(mask));
  else
    hipLaunchKernelGGL((preprocess_batch_kernel<OutT>), grid, dim3(256), 0, s, in, tab, nm, (int)H, (int)W,
                       static_cast<OutT*>(dst), static_cast<OutT*>(mask));
  return launched();
}

// codetr_preprocess_tiles_u8_*: the batch entry's checks with a crop per row, then preprocess_tiles_kernel
template <class OutT>
int launch_pre_tiles(void* stream, const void* src, int64_t src_bytes, int64_t N, const int64_t* tiles, int64_t H, int64_t W,
                     const float* mean, const float* stdv, const int* pad, float pad_fill, void* dst, void* mask) {
  if (!src || !tiles || !mean || !stdv || !pad || !dst || src_bytes <= 0 || N <= 0 || H <= 0 || W <= 0)
    return CODETR_E_BADARG;
  if (N > kPreBatchMax || H > 65535 || W > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  TileTable tab = {};
  BatchNorm nm;
  if (const int rc = pre_norm_args(mean, stdv, pad, pad_fill, nm)) return rc;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = tiles + 11 * n;  // src_offset, H_img, W_img, y0, x0, H_crop, W_crop, H_resized, W_resized, H_pad, W_pad
    const int64_t off = r[0], Hi = r[1], Wi = r[2], y0 = r[3], x0 = r[4], Hc = r[5], Wc = r[6], Hr = r[7], Wr = r[8],
                  Hp = r[9], Wp = r[10];
    if (off < 0 || Hi <= 0 || Wi <= 0 || y0 < 0 || x0 < 0 || Hc <= 0 || Wc <= 0 || Hr <= 0 || Wr <= 0 || Hp < Hr ||
        Wp < Wr || Hp > H || Wp > W)
      return CODETR_E_BADARG;
    if (Hi > 32767 || Wi > 32767) return CODETR_E_TOO_LARGE;
    if (y0 > Hi || Hc > Hi - y0 || x0 > Wi || Wc > Wi - x0) return CODETR_E_BADARG;  // the crop must lie in the image,
    if (off > src_bytes || Hi * Wi * 3 > src_bytes - off) return CODETR_E_BADARG;    // the image in the buffer
    tab.img[n] = TileImage{off + (y0 * Wi + x0) * 3, (int)Wi, (int)Hc, (int)Wc, (int)Hr, (int)Wr, (int)Hp, (int)Wp};
  }
  hipLaunchKernelGGL((preprocess_tiles_kernel<OutT>), dim3((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)N), dim3(256),
                     0, static_cast<hipStream_t>(stream), static_cast<const unsigned char*>(src), tab, nm, (int)H, (int)W,
                     static_cast<OutT*>(dst), static_cast<OutT*>(mask));
  return launched();
}

template <class T>
int launch_post(void* stream, const void* boxes, const void* scores, const int64_t* labels, const void* divisors,
                int64_t N, int64_t Q, int apply_threshold, float score_threshold, int apply_nms, float iou_threshold,
                void* boxes_out, void* scores_out, int64_t* labels_out, int* count) {
  if (!boxes || !scores || !labels || !divisors || !boxes_out || !scores_out || !labels_out || !count || N <= 0 ||
      Q <= 0)
    return CODETR_E_BADARG;
  if (Q > kPostMaxQ || N > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  hipLaunchKernelGGL((postprocess_kernel<T>), dim3((unsigned)N), dim3(kPostMaxQ), 0, static_cast<hipStream_t>(stream),
                     static_cast<const T*>(boxes), static_cast<const T*>(scores), labels,
                     static_cast<const T*>(divisors), (int)Q, apply_threshold ? 1 : 0, score_threshold,
                     apply_nms ? 1 : 0, iou_threshold, static_cast<T*>(boxes_out), static_cast<T*>(scores_out),
                     labels_out, count);
  return launched();
}

template <class T>
int launch_softnms(void* stream, const void* boxes, const void* scores, const int64_t* labels, const void* divisors,
                   int64_t N, int64_t Q, int apply_threshold, float score_threshold, int method, float iou_threshold,
                   float min_score, int64_t max_keep, void* boxes_out, void* scores_out, int64_t* labels_out,
                   int* index_out, int* count) {
  if (!boxes || !scores || !labels || !divisors || !boxes_out || !scores_out || !labels_out || !index_out || !count ||
      N <= 0 || Q <= 0)
    return CODETR_E_BADARG;
  if (method != CODETR_SOFTNMS_NAIVE && method != CODETR_SOFTNMS_LINEAR) return CODETR_E_BADARG;
  if (!__builtin_isfinite(iou_threshold) || !__builtin_isfinite(min_score)) return CODETR_E_BADARG;
  if (Q > kPostMaxQ || N > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  const int keep = max_keep <= 0 || max_keep > Q ? 0 : (int)max_keep;
  hipLaunchKernelGGL((postprocess_softnms_kernel<T>), dim3((unsigned)N), dim3(kNmsThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                     labels, static_cast<const T*>(divisors), (int)Q, apply_threshold ? 1 : 0, score_threshold,
                     method == CODETR_SOFTNMS_LINEAR ? 1 : 0, iou_threshold, min_score, keep, static_cast<T*>(boxes_out),
                     static_cast<T*>(scores_out), labels_out, index_out, count);
  return launched();
}

template <class T>
int launch_tta_merge(void* stream, const void* boxes, const void* scores, const int64_t* labels, const int* count,
                     int64_t V, int64_t N, int64_t Q, uint32_t flip_mask, const float* width, int mode,
                     float iou_threshold, float min_score, int64_t max_keep, void* boxes_out, void* scores_out,
                     int64_t* labels_out, int* index_out, int* count_out) {
  if (!boxes || !scores || !labels || !count || !width || !boxes_out || !scores_out || !labels_out || !index_out ||
      !count_out || V <= 0 || N <= 0 || Q <= 0)
    return CODETR_E_BADARG;
  if (mode != CODETR_TTA_NMS_HARD && mode != CODETR_TTA_NMS_SOFT_NAIVE && mode != CODETR_TTA_NMS_SOFT_LINEAR)
    return CODETR_E_BADARG;
  if (!__builtin_isfinite(iou_threshold) || !__builtin_isfinite(min_score)) return CODETR_E_BADARG;
  if (V < 32 && (flip_mask >> V) != 0u) return CODETR_E_BADARG;  // a flip bit of a view that does not exist
  if (V > CODETR_TTA_MAX_VIEWS || Q > kTtaMaxC || V * Q > kTtaMaxC || N > 0x7fffffffLL / kTtaMaxC ||
      max_keep > 0x7fffffffLL)
    return CODETR_E_TOO_LARGE;
  const int C = (int)(V * Q);
  int P = 1;
  while (P < C) P <<= 1;
  if (const hipError_t e = allow_large_lds<tta_merge_kernel<T>>((int)tta_lds_bytes(kTtaMaxC)); e != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL((tta_merge_kernel<T>), dim3((unsigned)N), dim3(kNmsThreads), tta_lds_bytes(P),
                     static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                     labels, count, (int)V, (int)N, (int)Q, P, flip_mask, width, mode, iou_threshold, min_score,
                     max_keep > 0 ? (int)max_keep : 0, max_keep > 0 ? (int)max_keep : C, static_cast<T*>(boxes_out),
                     static_cast<T*>(scores_out), labels_out, index_out, count_out);
  return launched();
}

template <class T>
int launch_slice_merge(void* stream, const void* boxes, const void* scores, const int64_t* labels, const int* count,
                       const int* rows, const float* origin, const float* size, int64_t R, int64_t N, int64_t V, int64_t Q,
                       int metric, int mode, float threshold, int class_agnostic, int64_t max_keep, void* boxes_out,
                       void* scores_out, int64_t* labels_out, int* index_out, int* count_out) {
  if (!boxes || !scores || !labels || !count || !rows || !origin || !size || !boxes_out || !scores_out || !labels_out ||
      !index_out || !count_out || R <= 0 || N <= 0 || V <= 0 || Q <= 0)
    return CODETR_E_BADARG;
  if (metric != CODETR_SLICE_IOU && metric != CODETR_SLICE_IOS) return CODETR_E_BADARG;
  if (mode != CODETR_SLICE_NMS && mode != CODETR_SLICE_NMM) return CODETR_E_BADARG;
  if (!__builtin_isfinite(threshold)) return CODETR_E_BADARG;
  if (V > kSliceMaxV || Q > kTtaMaxC || V * Q > kTtaMaxC || N > 0x7fffffffLL / kTtaMaxC || R > 0x7fffffffLL / kTtaMaxC ||
      max_keep > 0x7fffffffLL)
    return CODETR_E_TOO_LARGE;
  const int C = (int)(V * Q);
  int P = 1;
  while (P < C) P <<= 1;
  if (const hipError_t e = allow_large_lds<slice_merge_kernel<T>>((int)tta_lds_bytes(kTtaMaxC)); e != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL((slice_merge_kernel<T>), dim3((unsigned)N), dim3(kNmsThreads), tta_lds_bytes(P),
                     static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                     labels, count, rows, origin, size, (int)R, (int)V, (int)Q, P, metric, mode, threshold,
                     class_agnostic ? 1 : 0, max_keep > 0 ? (int)max_keep : 0, max_keep > 0 ? (int)max_keep : C,
                     static_cast<T*>(boxes_out), static_cast<T*>(scores_out), labels_out, index_out, count_out);
  return launched();
}

template <class T>
int launch_wbf_merge(void* stream, const void* boxes, const void* scores, const int64_t* labels, const int* count,
                     int64_t V, int64_t N, int64_t Q, uint32_t flip_mask, const float* width, const float* weights,
                     int conf_type, float iou_threshold, float skip_box_thr, int64_t max_keep, void* boxes_out,
                     void* scores_out, int64_t* labels_out, int* index_out, int* count_out, int* votes_out) {
  if (!boxes || !scores || !labels || !count || !width || !boxes_out || !scores_out || !labels_out || !index_out ||
      !count_out || !votes_out || V <= 0 || N <= 0 || Q <= 0)
    return CODETR_E_BADARG;
  if (conf_type != CODETR_WBF_CONF_AVG && conf_type != CODETR_WBF_CONF_MAX) return CODETR_E_BADARG;
  if (!__builtin_isfinite(iou_threshold) || !__builtin_isfinite(skip_box_thr)) return CODETR_E_BADARG;
  if (V < 32 && (flip_mask >> V) != 0u) return CODETR_E_BADARG;  // a flip bit of a view that does not exist
  if (V > CODETR_TTA_MAX_VIEWS || Q > kTtaMaxC || V * Q > kTtaMaxC || N > 0x7fffffffLL / kTtaMaxC ||
      max_keep > 0x7fffffffLL)
    return CODETR_E_TOO_LARGE;
  WbfWeights wt = {};
  float wsum = 0.f, wmax = 0.f;
  for (int v = 0; v < (int)V; ++v) {
    const float w = weights ? weights[v] : 1.f;
    if (!__builtin_isfinite(w) || !(w > 0.f)) return CODETR_E_BADARG;
    wt.w[v] = w;
    wsum = wsum + w;  // in view order, one rounding per addition
    wmax = w > wmax ? w : wmax;
  }
  const int C = (int)(V * Q);
  int P = 1;
  while (P < C) P <<= 1;
  if (const hipError_t e = allow_large_lds<wbf_merge_kernel<T>>((int)tta_lds_bytes(kTtaMaxC)); e != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL((wbf_merge_kernel<T>), dim3((unsigned)N), dim3(kNmsThreads), tta_lds_bytes(P),
                     static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                     labels, count, (int)V, (int)N, (int)Q, P, flip_mask, width, wt, wsum, wmax,
                     conf_type == CODETR_WBF_CONF_MAX ? 1 : 0, iou_threshold, skip_box_thr,
                     max_keep > 0 ? (int)max_keep : 0, max_keep > 0 ? (int)max_keep : C, static_cast<T*>(boxes_out),
                     static_cast<T*>(scores_out), labels_out, index_out, count_out, votes_out);
  return launched();
}

}  // namespace

extern "C" {

int codetr_preprocess_u8_f16(void* stream, const void* src_dev, int64_t H_src, int64_t W_src, int64_t H_resized,
                             int64_t W_resized, int64_t H_pad, int64_t W_pad, const float* mean_host,
                             const float* std_host, const int* pad_value_host, void* dst_dev, void* mask_dev) {
  return launch_pre<_Float16>(stream, src_dev, H_src, W_src, H_resized, W_resized, H_pad, W_pad, mean_host, std_host,
                              pad_value_host, dst_dev, mask_dev);
}

int codetr_preprocess_u8_f32(void* stream, const void* src_dev, int64_t H_src, int64_t W_src, int64_t H_resized,
                             int64_t W_resized, int64_t H_pad, int64_t W_pad, const float* mean_host,
                             const float* std_host, const int* pad_value_host, void* dst_dev, void* mask_dev) {
  return launch_pre<float>(stream, src_dev, H_src, W_src, H_resized, W_resized, H_pad, W_pad, mean_host, std_host,
                           pad_value_host, dst_dev, mask_dev);
}

int codetr_batched_nms_f32(void* stream, const float* boxes_sorted_dev, const int64_t* labels_sorted_dev, int64_t N,
                           float iou_threshold, void* keep_dev) {
  if (N == 0) return 0;
  if (!boxes_sorted_dev || !labels_sorted_dev || !keep_dev || N < 0) return CODETR_E_BADARG;
  if (N > 60000) return CODETR_E_TOO_LARGE;  // keep flags live in LDS
  const int threads = N >= 1024 ? 1024 : (int)((N + 63) / 64 * 64);
  hipLaunchKernelGGL(batched_nms_kernel, dim3(1), dim3(threads), (size_t)((N + 15) / 16 * 16),
                     static_cast<hipStream_t>(stream), boxes_sorted_dev, labels_sorted_dev, (int)N, iou_threshold,
                     static_cast<unsigned char*>(keep_dev));
  return launched();
}

// STEM_f16 / STEM_bf16 / STEM_f32 (PARAMS) = LAUNCH<element type> ARGS
#define CODETR_ENTRIES(STEM, LAUNCH, PARAMS, ARGS)            \
  int STEM##_f16 PARAMS { return LAUNCH<_Float16> ARGS; }     \
  int STEM##_bf16 PARAMS { return LAUNCH<Bf16> ARGS; }        \
  int STEM##_f32 PARAMS { return LAUNCH<float> ARGS; }

CODETR_ENTRIES(codetr_preprocess_batch_u8, launch_pre_rows,
               (void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* images_host, int64_t H,
                int64_t W, const float* mean_host, const float* std_host, const int* pad_value_host, float pad_fill,
                void* dst_dev, void* mask_dev),
               (7, stream, src_dev, src_bytes, N, images_host, H, W, mean_host, std_host, pad_value_host, pad_fill, dst_dev,
                mask_dev))

CODETR_ENTRIES(codetr_preprocess_views_u8, launch_pre_rows,
               (void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* images_host, int64_t H,
                int64_t W, const float* mean_host, const float* std_host, const int* pad_value_host, float pad_fill,
                void* dst_dev, void* mask_dev),
               (8, stream, src_dev, src_bytes, N, images_host, H, W, mean_host, std_host, pad_value_host, pad_fill, dst_dev,
                mask_dev))

CODETR_ENTRIES(codetr_postprocess_detections, launch_post,
               (void* stream, const void* boxes_dev, const void* scores_dev, const int64_t* labels_dev,
                const void* divisor_dev, int64_t N, int64_t Q, int apply_threshold, float score_threshold, int apply_nms,
                float iou_threshold, void* boxes_out_dev, void* scores_out_dev, int64_t* labels_out_dev, int* count_dev),
               (stream, boxes_dev, scores_dev, labels_dev, divisor_dev, N, Q, apply_threshold, score_threshold, apply_nms,
                iou_threshold, boxes_out_dev, scores_out_dev, labels_out_dev, count_dev))

CODETR_ENTRIES(codetr_postprocess_softnms, launch_softnms,
               (void* stream, const void* boxes_dev, const void* scores_dev, const int64_t* labels_dev,
                const void* divisor_dev, int64_t N, int64_t Q, int apply_threshold, float score_threshold, int method,
                float iou_threshold, float min_score, int64_t max_keep, void* boxes_out_dev, void* scores_out_dev,
                int64_t* labels_out_dev, int* index_out_dev, int* count_dev),
               (stream, boxes_dev, scores_dev, labels_dev, divisor_dev, N, Q, apply_threshold, score_threshold, method,
                iou_threshold, min_score, max_keep, boxes_out_dev, scores_out_dev, labels_out_dev, index_out_dev,
                count_dev))

CODETR_ENTRIES(codetr_tta_merge, launch_tta_merge,
               (void* stream, const void* boxes_dev, const void* scores_dev, const int64_t* labels_dev,
                const int* count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask, const float* width_dev,
                int mode, float iou_threshold, float min_score, int64_t max_keep, void* boxes_out_dev,
                void* scores_out_dev, int64_t* labels_out_dev, int* index_out_dev, int* count_out_dev),
               (stream, boxes_dev, scores_dev, labels_dev, count_dev, V, N, Q, flip_mask, width_dev, mode, iou_threshold,
                min_score, max_keep, boxes_out_dev, scores_out_dev, labels_out_dev, index_out_dev, count_out_dev))

CODETR_ENTRIES(codetr_preprocess_tiles_u8, launch_pre_tiles,
               (void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* tiles_host, int64_t H,
                int64_t W, const float* mean_host, const float* std_host, const int* pad_value_host, float pad_fill,
                void* dst_dev, void* mask_dev),
               (stream, src_dev, src_bytes, N, tiles_host, H, W, mean_host, std_host, pad_value_host, pad_fill, dst_dev,
                mask_dev))

CODETR_ENTRIES(codetr_slice_merge, launch_slice_merge,
               (void* stream, const void* boxes_dev, const void* scores_dev, const int64_t* labels_dev,
                const int* count_dev, const int* rows_dev, const float* origin_dev, const float* size_dev, int64_t R,
                int64_t N, int64_t V, int64_t Q, int metric, int mode, float threshold, int class_agnostic,
                int64_t max_keep, void* boxes_out_dev, void* scores_out_dev, int64_t* labels_out_dev,
                int* index_out_dev, int* count_out_dev),
               (stream, boxes_dev, scores_dev, labels_dev, count_dev, rows_dev, origin_dev, size_dev, R, N, V, Q, metric,
                mode, threshold, class_agnostic, max_keep, boxes_out_dev, scores_out_dev, labels_out_dev, index_out_dev,
                count_out_dev))
int codetr_wbf_abi_version(void) { return CODETR_WBF_ABI_VERSION; }

CODETR_ENTRIES(codetr_wbf_merge, launch_wbf_merge,
               (void* stream, const void* boxes_dev, const void* scores_dev, const int64_t* labels_dev,
                const int* count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask, const float* width_dev,
                const float* weights_host, int conf_type, float iou_threshold, float skip_box_thr, int64_t max_keep,
                void* boxes_out_dev, void* scores_out_dev, int64_t* labels_out_dev, int* index_out_dev,
                int* count_out_dev, int* votes_out_dev),
               (stream, boxes_dev, scores_dev, labels_dev, count_dev, V, N, Q, flip_mask, width_dev, weights_host,
                conf_type, iou_threshold, skip_box_thr, max_keep, boxes_out_dev, scores_out_dev, labels_out_dev,
                index_out_dev, count_out_dev, votes_out_dev))
#undef CODETR_ENTRIES

}  // extern "C"
