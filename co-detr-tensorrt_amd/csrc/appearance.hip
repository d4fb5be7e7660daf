// The colour descriptors of include/codetr_appearance.h: codetr_appearance_describe_*.
//
// appearance_describe_kernel  one wave per detection, four per workgroup.  A lane takes 8 of the 512 samples (its column
//                             i = lane & 15 is fixed, its rows are (lane >> 4) + 4 k), gathers the three bytes of each
//                             pixel and adds 1 to one of the wave's 128 counters in LDS (LDS atomics: the lanes of a wave
//                             collide freely on a solid-colour object, and the LDS unit serialises them without a loop).
//                             The row goes out as one coalesced 256-byte store, two counters per lane.
// fp32 with one rounding per operation: contraction is off for the whole file.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_appearance.h"
#include "box_prims.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = CODETR_APPEARANCE_BINS;
static_assert(CODETR_APPEARANCE_COLS * CODETR_APPEARANCE_ROWS == 8 * 64, "eight samples per lane");
static_assert(kBins == 2 * 64, "two counters per lane");

struct ImageTable {  // a kernel argument: byte offset, H, W of every image
  int64_t off[CODETR_PREPROCESS_BATCH_MAX];
  int H[CODETR_PREPROCESS_BATCH_MAX], W[CODETR_PREPROCESS_BATCH_MAX];
};

template <class T>
__global__ __launch_bounds__(kThreads) void appearance_describe_kernel(const unsigned char* __restrict__ src, ImageTable tab,
                                                                       const T* __restrict__ boxes,
                                                                       const int* __restrict__ count, int N, int Q,
                                                                       unsigned* __restrict__ desc_out) {
  __shared__ int hist[kWaves][kBins];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t det = (int64_t)blockIdx.x * kWaves + wave;  // (wave-uniform)
  const bool have = det < (int64_t)N * Q;
  hist[wave][lane] = 0, hist[wave][lane + 64] = 0;
  __syncthreads();
  if (have) {
    const int n = (int)(det / Q), j = (int)(det % Q);
    const int cnt = min(max(count[n], 0), Q);
    const T* bp = boxes + det * 4;
    const float x1 = to_f32(bp[0]), y1 = to_f32(bp[1]), x2 = to_f32(bp[2]), y2 = to_f32(bp[3]);
    const float w = x2 - x1, h = y2 - y1;
    const bool finite =
        __builtin_isfinite(x1) && __builtin_isfinite(y1) && __builtin_isfinite(x2) && __builtin_isfinite(y2);
    if (j < cnt && finite && w > 0.f && h > 0.f) {
      const int H = tab.H[n], W = tab.W[n];
      const unsigned char* img = src + tab.off[n];
      const float u = (float)(6 * (lane & 15) + 19) / 128.0f;
      const float x = x1 + w * u;
      const int px = (int)fminf(fmaxf(floorf(x), 0.0f), (float)(W - 1));
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int r = (lane >> 4) + 4 * k;
        const float v = (float)(6 * r + 35) / 256.0f;
        const float y = y1 + h * v;
        const int py = (int)fminf(fmaxf(floorf(y), 0.0f), (float)(H - 1));
        const unsigned char* p = img + ((int64_t)py * W + px) * 3;  // inside the image: 0 <= px < W, 0 <= py < H
        const int R = p[0], G = p[1], B = p[2];
        atomicAdd(&hist[wave][(r >> 4) * 64 + (R >> 6) * 16 + (G >> 6) * 4 + (B >> 6)], 1);
      }
    }
  }
  __syncthreads();
  if (have) desc_out[det * (kBins / 2) + lane] = (unsigned)hist[wave][2 * lane] | ((unsigned)hist[wave][2 * lane + 1] << 16);
}

template <class T>
int launch_describe(void* stream, const void* src, int64_t src_bytes, int64_t N, const int64_t* rows, const void* boxes,
                    const int* count, int64_t Q, uint16_t* desc_out) {
  if (!src || !rows || !boxes || !count || !desc_out || src_bytes <= 0 || N <= 0 || Q <= 0 || ((uintptr_t)desc_out & 3u))
    return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX || Q > CODETR_POSTPROCESS_MAX_Q) return CODETR_E_TOO_LARGE;
  ImageTable tab = {};
  for (int64_t n = 0; n < N; ++n) {
    const int64_t off = rows[3 * n], H = rows[3 * n + 1], W = rows[3 * n + 2];
    if (H <= 0 || W <= 0 || off < 0) return CODETR_E_BADARG;
    if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (off > src_bytes || H * W * 3 > src_bytes - off) return CODETR_E_BADARG;
    tab.off[n] = off, tab.H[n] = (int)H, tab.W[n] = (int)W;
  }
  const unsigned groups = (unsigned)((N * Q + kWaves - 1) / kWaves);
  hipLaunchKernelGGL((appearance_describe_kernel<T>), dim3(groups), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned char*>(src), tab, static_cast<const T*>(boxes), count, (int)N, (int)Q,
                     reinterpret_cast<unsigned*>(desc_out));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

extern "C" {

int codetr_appearance_abi_version(void) { return CODETR_APPEARANCE_ABI_VERSION; }
int64_t codetr_appearance_state_bytes(int64_t max_tracks) {
  if (max_tracks <= 0 || max_tracks > CODETR_TRACK_MAX_TRACKS) return CODETR_E_BADARG;
  return 2 * kBins * max_tracks;
}
int64_t codetr_appearance_work_bytes(int64_t S, int64_t max_tracks, int64_t Q) {
  if (S <= 0 || S > 0x7fffffffLL || max_tracks <= 0 || max_tracks > CODETR_TRACK_MAX_TRACKS || Q <= 0 ||
      Q > CODETR_POSTPROCESS_MAX_Q)
    return CODETR_E_BADARG;
  return 4 * S * max_tracks * Q;
}

#define CODETR_DESCRIBE_ENTRY(SUFFIX, TYPE)                                                                               \
  int codetr_appearance_describe_##SUFFIX(void* stream, const void* src_dev, int64_t src_bytes, int64_t N,                \
                                          const int64_t* rows_host, const void* boxes_dev, const int* count_dev,          \
                                          int64_t Q, uint16_t* desc_out_dev) {                                            \
    return launch_describe<TYPE>(stream, src_dev, src_bytes, N, rows_host, boxes_dev, count_dev, Q, desc_out_dev);        \
  }
CODETR_DESCRIBE_ENTRY(f16, _Float16)
CODETR_DESCRIBE_ENTRY(bf16, Bf16)
CODETR_DESCRIBE_ENTRY(f32, float)
#undef CODETR_DESCRIBE_ENTRY

}  // extern "C"
