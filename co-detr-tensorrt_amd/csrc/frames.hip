// The Inferencer's input side on the GPU: frames as decoders and capture libraries hand them out -- packed RGB / BGR /
// RGBA / BGRA / GRAY, NV12 / NV21 and I420, every plane with a byte offset and a row pitch of its own -- converted to
// the packed RGB HWC images every kernel of prepost.hip and draw.hip reads.  The arithmetic is stated in integers in
// include/codetr_hip.h ("Frames").
//
// frames_to_rgb_kernel  one thread per 4 consecutive pixels of a row (two chroma pairs, 12 output bytes); grid
//                     (ceil(ceil(Wmax / 4) / 256), Hmax, N), the frame's table entry read with a uniform index.  The
//                     kernel is bandwidth-bound (1 to 4 bytes read and 3 written per pixel): a thread's bytes of a plane
//                     row come in as whole dwords when all of them lie in the row and the address is 4-byte aligned, byte
//                     by byte otherwise (row tails, odd offsets and pitches) -- into the same packed little-endian words,
//                     which the one decoder then reads, so both ways give the same bytes.  The 12 output bytes leave as
//                     three dwords when the thread has 4 pixels and its address is aligned (every row of an image whose
//                     offset is a multiple of 4 and whose width is one too), byte by byte otherwise.  Nothing outside a
//                     declared plane row is read and nothing outside an output image is written.  No LDS, no scratch.
// A separate translation unit from prepost.hip on purpose: the code of the kernels there is pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "device_prims.h"

namespace {

constexpr int kPix = 4;        // pixels per thread
constexpr int kThreads = 256;  // threads per workgroup: 1024 pixels of one row

struct Frame {
  int64_t off[3], pitch[3], dst;
  int fmt, H, W;
};
struct FrameTable {  // a kernel argument, like prepost.hip's BatchTable
  Frame f[CODETR_PREPROCESS_BATCH_MAX];
};
struct YuvCoef {
  int cy, crv, cgu, cgv, cbu, y0;
};

// dwords whose alignment is 4 bytes whatever their count: the rows of a plane promise no more
typedef unsigned u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// `nbytes` (<= 4 * NW) bytes at p -> NW little-endian words, the bytes beyond nbytes zero.  Reads exactly those bytes.
template <int NW>
__device__ __forceinline__ void load_words(const unsigned char* __restrict__ p, int nbytes, unsigned (&w)[NW]) {
  if (nbytes == 4 * NW && aligned4(p)) {
    if constexpr (NW == 1) {
      w[0] = *reinterpret_cast<const unsigned*>(p);
    } else if constexpr (NW == 3) {
      const u32x3_a4 v = *reinterpret_cast<const u32x3_a4*>(p);
      w[0] = v.x, w[1] = v.y, w[2] = v.z;
    } else {
      static_assert(NW == 4, "1, 3 or 4 words");
      const u32x4_a4 v = *reinterpret_cast<const u32x4_a4*>(p);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = 0;
  if (nbytes == 4 * NW) {  // all of them, unaligned: independent byte loads, one wait
#pragma unroll
    for (int k = 0; k < 4 * NW; ++k) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
    return;
  }
#pragma unroll
  for (int k = 0; k < 4 * NW; ++k)
    if (k < nbytes) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
}

// one or two bytes (an I420 chroma row has one sample per two pixels)
__device__ __forceinline__ unsigned load_half(const unsigned char* __restrict__ p, int nbytes) {
  if (nbytes == 2 && ((uintptr_t)p & 1u) == 0) return *reinterpret_cast<const unsigned short*>(p);
  unsigned v = p[0];
  if (nbytes == 2) v |= (unsigned)p[1] << 8;
  return v;
}

template <int NW>
__device__ __forceinline__ int byte_of(const unsigned (&w)[NW], int k) {  // k is a compile-time constant at every use
  return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ void yuv_to_rgb(int Y, int U, int V, const YuvCoef& k, int (&rgb)[3]) {
  const int c = max(0, Y - k.y0), d = U - 128, e = V - 128;
  const int yy = k.cy * c + (1 << 19);
  rgb[0] = clamp255((yy + k.crv * e) >> 20);
  rgb[1] = clamp255((yy + k.cgu * d + k.cgv * e) >> 20);
  rgb[2] = clamp255((yy + k.cbu * d) >> 20);
}

// packed 1-plane formats: BPP bytes per pixel, red at byte RED and blue at byte 2 - RED of a pixel (GRAY: BPP 1)
template <int BPP, int RED>
__device__ __forceinline__ void load_packed(const unsigned char* __restrict__ src, const Frame& fr, int y, int x0, int npx,
                                            int (&px)[kPix][3]) {
  unsigned w[BPP];
  load_words<BPP>(src + fr.off[0] + (int64_t)y * fr.pitch[0] + (int64_t)x0 * BPP, npx * BPP, w);
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    if constexpr (BPP == 1) {
      px[i][0] = px[i][1] = px[i][2] = byte_of(w, i);
    } else {
      px[i][0] = byte_of(w, BPP * i + RED);
      px[i][1] = byte_of(w, BPP * i + 1);
      px[i][2] = byte_of(w, BPP * i + 2 - RED);
    }
  }
}

// NV12 (UFIRST 1) / NV21 (UFIRST 0): the chroma pair of pixel (y, x) is pair x >> 1 of chroma row y >> 1
template <int UFIRST>
__device__ __forceinline__ void load_nv(const unsigned char* __restrict__ src, const Frame& fr, int y, int x0, int npx,
                                        const YuvCoef& k, int (&px)[kPix][3]) {
  unsigned wy[1], wc[1];
  load_words<1>(src + fr.off[0] + (int64_t)y * fr.pitch[0] + x0, npx, wy);
  load_words<1>(src + fr.off[1] + (int64_t)(y >> 1) * fr.pitch[1] + x0, 2 * ((npx + 1) >> 1), wc);
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    const int a = byte_of(wc, 2 * (i >> 1)), b = byte_of(wc, 2 * (i >> 1) + 1);
    yuv_to_rgb(byte_of(wy, i), UFIRST ? a : b, UFIRST ? b : a, k, px[i]);
  }
}

__device__ __forceinline__ void load_i420(const unsigned char* __restrict__ src, const Frame& fr, int y, int x0, int npx,
                                          const YuvCoef& k, int (&px)[kPix][3]) {
  unsigned wy[1];
  load_words<1>(src + fr.off[0] + (int64_t)y * fr.pitch[0] + x0, npx, wy);
  const int nc = (npx + 1) >> 1;
  const unsigned wu[1] = {load_half(src + fr.off[1] + (int64_t)(y >> 1) * fr.pitch[1] + (x0 >> 1), nc)};
  const unsigned wv[1] = {load_half(src + fr.off[2] + (int64_t)(y >> 1) * fr.pitch[2] + (x0 >> 1), nc)};
#pragma unroll
  for (int i = 0; i < kPix; ++i) yuv_to_rgb(byte_of(wy, i), byte_of(wu, i >> 1), byte_of(wv, i >> 1), k, px[i]);
}

// grid (ceil(ceil(Wmax / 4) / 256), Hmax, N)
__global__ __launch_bounds__(kThreads) void frames_to_rgb_kernel(const unsigned char* __restrict__ src, FrameTable tab,
                                                                 YuvCoef k, unsigned char* __restrict__ dst) {
  const Frame& fr = tab.f[blockIdx.z];  // (uniform: the entry comes through the scalar cache)
  const int y = blockIdx.y;
  const int x0 = (blockIdx.x * kThreads + threadIdx.x) * kPix;
  if (y >= fr.H || x0 >= fr.W) return;
  const int npx = min(kPix, fr.W - x0);

  int px[kPix][3];
  switch (fr.fmt) {  // (uniform)
    case CODETR_FRAME_RGB: load_packed<3, 0>(src, fr, y, x0, npx, px); break;
    case CODETR_FRAME_BGR: load_packed<3, 2>(src, fr, y, x0, npx, px); break;
    case CODETR_FRAME_RGBA: load_packed<4, 0>(src, fr, y, x0, npx, px); break;
    case CODETR_FRAME_BGRA: load_packed<4, 2>(src, fr, y, x0, npx, px); break;
    case CODETR_FRAME_GRAY: load_packed<1, 0>(src, fr, y, x0, npx, px); break;
    case CODETR_FRAME_NV12: load_nv<1>(src, fr, y, x0, npx, k, px); break;
    case CODETR_FRAME_NV21: load_nv<0>(src, fr, y, x0, npx, k, px); break;
    default: load_i420(src, fr, y, x0, npx, k, px); break;
  }

  unsigned char* q = dst + fr.dst + ((int64_t)y * fr.W + x0) * 3;
  if (npx == kPix && aligned4(q)) {
    u32x3_a4 o;
    o.x = (unsigned)px[0][0] | (unsigned)px[0][1] << 8 | (unsigned)px[0][2] << 16 | (unsigned)px[1][0] << 24;
    o.y = (unsigned)px[1][1] | (unsigned)px[1][2] << 8 | (unsigned)px[2][0] << 16 | (unsigned)px[2][1] << 24;
    o.z = (unsigned)px[2][2] | (unsigned)px[3][0] << 8 | (unsigned)px[3][1] << 16 | (unsigned)px[3][2] << 24;
    *reinterpret_cast<u32x3_a4*>(q) = o;
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      if (i < npx) {
        q[3 * i] = (unsigned char)px[i][0];
        q[3 * i + 1] = (unsigned char)px[i][1];
        q[3 * i + 2] = (unsigned char)px[i][2];
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

const int kCoef[2][2][5] = {{CODETR_YUV_BT601_LIMITED, CODETR_YUV_BT601_FULL},
                            {CODETR_YUV_BT709_LIMITED, CODETR_YUV_BT709_FULL}};

// rows of `rb` bytes, `rows` of them `pitch` apart from `off`: all inside [0, total)
bool rows_inside(int64_t off, int64_t pitch, int64_t rb, int64_t rows, int64_t total) {
  if (off > total || rb > total - off) return false;
  return rows == 1 || pitch <= (total - off - rb) / (rows - 1);
}

}  // namespace

extern "C" int codetr_frames_to_rgb_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N,
                                       const int64_t* frames_host, int matrix, int range, void* dst_dev,
                                       int64_t dst_bytes) {
  if (!src_dev || !frames_host || !dst_dev || src_bytes <= 0 || dst_bytes <= 0 || N <= 0) return CODETR_E_BADARG;
  if ((matrix != CODETR_COLOR_BT601 && matrix != CODETR_COLOR_BT709) ||
      (range != CODETR_COLOR_LIMITED && range != CODETR_COLOR_FULL))
    return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  FrameTable tab = {};
  int64_t Hmax = 0, Wmax = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = frames_host + 10 * n;
    const int64_t fmt = r[0], H = r[1], W = r[2], dst = r[9];
    if (fmt < CODETR_FRAME_RGB || fmt > CODETR_FRAME_I420 || H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) return CODETR_E_TOO_LARGE;
    const int64_t ch = (H + 1) / 2, cw = (W + 1) / 2;
    int planes = 1;
    int64_t rb[3] = {W, 0, 0}, rows[3] = {H, ch, ch};
    switch (fmt) {
      case CODETR_FRAME_RGB:
      case CODETR_FRAME_BGR: rb[0] = 3 * W; break;
      case CODETR_FRAME_RGBA:
      case CODETR_FRAME_BGRA: rb[0] = 4 * W; break;
      case CODETR_FRAME_GRAY: break;
      case CODETR_FRAME_NV12:
      case CODETR_FRAME_NV21: planes = 2, rb[1] = 2 * cw; break;
      default: planes = 3, rb[1] = rb[2] = cw; break;
    }
    Frame& fr = tab.f[n];
    for (int p = 0; p < 3; ++p) {
      const int64_t off = r[3 + 2 * p], pitch = r[4 + 2 * p];
      if (off < 0) return CODETR_E_BADARG;
      if (p >= planes) continue;  // an unused plane: never read
      if (pitch < rb[p] || !rows_inside(off, pitch, rb[p], rows[p], src_bytes)) return CODETR_E_BADARG;
      fr.off[p] = off;
      fr.pitch[p] = pitch;
    }
    if (dst < 0 || dst > dst_bytes || H * W * 3 > dst_bytes - dst) return CODETR_E_BADARG;
    for (int64_t m = 0; m < n; ++m) {  // two output images may not share a byte
      const int64_t o2 = tab.f[m].dst, e2 = o2 + (int64_t)tab.f[m].H * tab.f[m].W * 3;
      if (dst < e2 && o2 < dst + H * W * 3) return CODETR_E_BADARG;
    }
    fr.dst = dst;
    fr.fmt = (int)fmt;
    fr.H = (int)H;
    fr.W = (int)W;
    Hmax = H > Hmax ? H : Hmax;
    Wmax = W > Wmax ? W : Wmax;
  }
  const int* c = kCoef[matrix][range];
  const YuvCoef k = {c[0], c[1], c[2], c[3], c[4], range == CODETR_COLOR_LIMITED ? 16 : 0};
  const int64_t groups = (Wmax + kPix - 1) / kPix;
  const dim3 grid((unsigned)((groups + kThreads - 1) / kThreads), (unsigned)Hmax, (unsigned)N);
  hipLaunchKernelGGL(frames_to_rgb_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned char*>(src_dev), tab, k, static_cast<unsigned char*>(dst_dev));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}
