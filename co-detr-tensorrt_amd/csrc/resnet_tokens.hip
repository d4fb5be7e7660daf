// The two non-GEMM pieces of the native ResNet-50 backbone (mmdet ResNet, depth 50, style 'pytorch', frozen BN: the R50
// config's backbone, configs/co_dino_5scale_r50_lsj_8xb2_1x_coco.py:22-31):
//   * the stem's gather: the 7x7 / stride-2 / pad-3 convolution on the 3-channel NCHW image is a GEMM over overlapping
//     windows; this writes its left operand [B Ho Wo, kpad] with the (c, ky, kx) column order of
//     conv1.weight.view(64, 147), zero-padded to kpad columns (the overlapping-window form of codetr_patch_im2col_b16);
//     codetr_linear_* with the BN-folded weight and ReLU then produces the token-major stem map;
//   * the 3x3 / stride-2 / pad-1 max pool on that token-major map (F.max_pool2d(x, 3, 2, 1)).
// Both are pure 16-bit data movement (the pool compares but never rounds) and write with 16-byte vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "device_prims.h"

namespace {


// one thread = one 8-column piece of one output row; the 8 columns are gathered element by element (three channels
// and 7-wide windows: no two columns of a piece share a 16-byte source run that a vector load could fetch)
__global__ __launch_bounds__(256) void conv_im2col_nchw_kernel(const unsigned short* __restrict__ x,
                                                               unsigned short* __restrict__ out, int C, int H, int W,
                                                               int Ho, int Wo, int k, int stride, int pad, int kpad8,
                                                               long total_pieces) {
  const int kk = k * k, ncols = C * kk;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total_pieces; i += (long)gridDim.x * 256) {
    const int piece = (int)(i % kpad8);
    long t = i / kpad8;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = piece * 8 + e;
      if (col < ncols) {
        const int c = col / kk, rem = col - c * kk;
        const int ky = rem / k, kx = rem - ky * k;
        const int y = oy * stride - pad + ky, xx = ox * stride - pad + kx;
        if (y >= 0 && y < H && xx >= 0 && xx < W) v[e] = x[((b * C + c) * (long)H + y) * W + xx];
      }
    }
    *reinterpret_cast<u16x8*>(out + i * 8) = v;
  }
}

__device__ __forceinline__ float b16_to_f32(unsigned short bits, bool bf16) {
  return bf16 ? bf16_to_f32(bits) : HalfT::to_f32(bits);
}

// torch's rule (max_pool2d's CUDA kernels): start at -inf, scan the in-map taps row by row, take a value when it is
// greater or NaN -- so padding never wins, any NaN wins over numbers and the last NaN of the scan is the one returned.
// The winner's own 16 bits are stored: the result is exact.
__global__ __launch_bounds__(256) void maxpool_tokens_kernel(const unsigned short* __restrict__ x,
                                                             unsigned short* __restrict__ y, int H, int W, int C8,
                                                             int Ho, int Wo, int k, int stride, int pad, int bf16,
                                                             long total_pieces) {
  const unsigned short neg_inf = bf16 ? 0xff80u : 0xfc00u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total_pieces; i += (long)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    long t = i / C8;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    u16x8 best = {neg_inf, neg_inf, neg_inf, neg_inf, neg_inf, neg_inf, neg_inf, neg_inf};
    float bestf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bestf[e] = -__builtin_inff();
    for (int ky = 0; ky < k; ++ky) {
      const int yy = oy * stride - pad + ky;
      if (yy < 0 || yy >= H) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int xx = ox * stride - pad + kx;
        if (xx < 0 || xx >= W) continue;
        const u16x8 v = *reinterpret_cast<const u16x8*>(x + (((b * H + yy) * (long)W + xx) * C8 + c8) * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = b16_to_f32(v[e], bf16 != 0);
          if (f > bestf[e] || f != f) {
            bestf[e] = f;
            best[e] = v[e];
          }
        }
      }
    }
    *reinterpret_cast<u16x8*>(y + i * 8) = best;
  }
}

int64_t grid_for(int64_t pieces) {
  const int64_t blocks = (pieces + 255) / 256;
  return blocks > 256 * 64 ? 256 * 64 : blocks;
}

}  // namespace

extern "C" {

int codetr_conv_im2col_nchw_b16(void* stream, const void* x_dev, int64_t B, int C, int64_t H, int64_t W, int k,
                                int stride, int pad, int kpad, void* out_dev) {
  if (!x_dev || !out_dev || B <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0)
    return CODETR_E_BADARG;
  if (kpad % 8 != 0 || C * k * k > kpad) return CODETR_E_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(out_dev) & 15) return CODETR_E_BADARG;
  const int64_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return CODETR_E_BADARG;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  const int64_t pieces = B * Ho * Wo * (kpad / 8);
  hipLaunchKernelGGL(conv_im2col_nchw_kernel, dim3((unsigned)grid_for(pieces)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned short*>(x_dev),
                     static_cast<unsigned short*>(out_dev), C, (int)H, (int)W, (int)Ho, (int)Wo, k, stride, pad,
                     kpad / 8, (long)pieces);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

int codetr_maxpool_tokens_b16(void* stream, const void* x_dev, int64_t B, int64_t H, int64_t W, int64_t C, int k,
                              int stride, int pad, int is_bf16, void* y_dev) {
  if (!x_dev || !y_dev || B <= 0 || H <= 0 || W <= 0 || C <= 0) return CODETR_E_BADARG;
  if (k != 3 || stride != 2 || pad != 1 || C % 8 != 0 || (is_bf16 != 0 && is_bf16 != 1)) return CODETR_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(y_dev)) & 15) return CODETR_E_BADARG;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL || C > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  const int64_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const int64_t pieces = B * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(maxpool_tokens_kernel, dim3((unsigned)grid_for(pieces)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned short*>(x_dev),
                     static_cast<unsigned short*>(y_dev), (int)H, (int)W, (int)(C / 8), (int)Ho, (int)Wo, k, stride,
                     pad, is_bf16, (long)pieces);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // extern "C"
