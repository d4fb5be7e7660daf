// The output rule of every 16-bit GEMM of this directory, said once (gemm_tile128.hip, gemm_tile256.hip, gemm_xs.hip: the
// 128-tile, 256-tile, X-stationary and split-K kernels; gemm_persist.h: the two persistent kernels; gemm_fp8.hip: the activation of its 16-bit output).
// tests/epilogue_exact.py restates it in torch and tests/test_epilogue_exact_gpu.py holds every kernel to it bit for bit:
//
//     y = E(E(act(acc + bias)) + r)            E = ONE round-to-nearest-even to the storage type
//     act 3 ("relu_res"):  y = E(relu(E(acc + bias) + r))      (with no residual, act 3 is act 1)
//     row state 1: the linear output is 0 (+ r);  row state 2: it is E(act(bias)) (+ r)
//
// ACT: 0 none, 1 relu, 2 gelu (erf form), 3 relu after the residual (the ResNet bottleneck's
// relu(bn3(conv3(x)) + identity): the accumulator leaves without activation, the ReLU is applied to the sum with the
// residual -- the same two roundings as act 0 + residual, then the exact ReLU).  ReLU is x < 0 ? 0 : x: a NaN stays a NaN,
// like torch.relu.  The bias is in the accumulator before any of this (the kernels start their accumulators at it).
// A kernel keeps its own addressing, staging loop and store shape; the values come from here.  Two places write a piece
// of the rule out beside these helpers, because through a helper their kernels compiled to other instructions than
// before (profiles/r20_epilogue_isa_diff.txt is taken with them written out): the row-state block of the 128- and
// 256-tile kernels' staged path, and the residual on the persistent kernels' four packed values.
#pragma once
#include "device_prims.h"

namespace {

template <bool ON>
__device__ __forceinline__ float relu_if(float x) { return ON ? (x < 0.f ? 0.f : x) : x; }

// ---- act(acc + bias), fp32
template <int ACT, bool HAS_RES>
__device__ __forceinline__ float epi_act(float x) {
  if (ACT == 1 || (ACT == 3 && !HAS_RES)) x = x < 0.f ? 0.f : x;
  if (ACT == 2) x = gelu_erf(x);
  return x;
}
// two values at once on the packed GELU (the persistent kernels).  Same fp32 results as epi_act; what a fp16 STORE of them
// holds may differ in the last bit (device_prims.h, gelu_erf2)
template <int ACT, bool HAS_RES>
__device__ __forceinline__ f32x2 epi_act2(f32x2 x) {
  if (ACT == 1 || (ACT == 3 && !HAS_RES)) x = f32x2{x.x < 0.f ? 0.f : x.x, x.y < 0.f ? 0.f : x.y};
  if (ACT == 2) x = gelu_erf2(x);
  return x;
}

// ---- row states: `h` / `v`, the rounded linear output of a row of state `mk`, becomes what the state asks for.  State 2:
// the INPUT row counts as zeros (`memory * keep` ahead of enc_output), y = E(act(bias)); any other non-zero state:
// masked_fill(mask[..., None], 0) on the linear's output.  T: the operands' type (the bias is one), OT: the type the
// output is rounded to.  bias: in global memory or LDS, read at the element's column n only if has_bias.
// (The helpers of this header work in place or on scalars: a 16-byte vector passed and returned by value compiled to
// different instructions than the loop it replaced.)
template <class T, class OT, int ACT, bool HAS_RES>
__device__ __forceinline__ void epi_row_state(unsigned short& h, unsigned char mk, bool has_bias,
                                              const unsigned short* bias, int n) {
  if (mk) {
    h = 0;
    if (mk == 2) h = OT::from_f32(epi_act<ACT, HAS_RES>(has_bias ? T::to_f32(bias[n]) : 0.f));
  }
}
// ... on the 8 columns n .. n + 7 of a row
template <class T, class OT, int ACT, bool HAS_RES>
__device__ __forceinline__ void epi_row_state(s16x8& v, unsigned char mk, bool has_bias, const unsigned short* bias,
                                              int n) {
  if (mk == 2) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      v[e] = (short)OT::from_f32(epi_act<ACT, HAS_RES>(has_bias ? T::to_f32(bias[n + e]) : 0.f));
  } else if (mk) {
    v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}

// ---- the residual: E(v + r), 16-bit + 16-bit -> 16-bit, the two roundings of `identity + linear(x)` in the reference's
// 16-bit path; act 3 puts its ReLU on the sum
template <class T, int ACT>
__device__ __forceinline__ unsigned short epi_residual(unsigned short v, unsigned short r) {
  return T::from_f32(relu_if<ACT == 3>(T::to_f32(v) + T::to_f32(r)));
}
// first column of the 8 residual values a lane requests for its 8 columns n .. n + 7 (N % 8 == 0): a lane past the
// last column re-reads the last 8 (its outputs are never stored)
__device__ __forceinline__ int epi_residual_col(int n, int N) { return n + 8 <= N ? n : N - 8; }

// ---- head-major destination y[b][head][position][channel] of element (m, n): rows m = (b, position) with `rows` positions
// per b, columns n = (head, channel) with hd channels per head.  An 8-column chunk never straddles heads (hd % 8 == 0);
// 8 consecutive rows of one head are 8 * hd * 2 contiguous bytes.  Never carries a residual.
__device__ __forceinline__ size_t epi_head_major(int m, int n, int N, int rows, int hd) {
  const int bb = m / rows, pos = m - bb * rows;
  const int head = n / hd, ch = n - head * hd;
  return (((size_t)bb * (N / hd) + head) * rows + pos) * hd + ch;
}

// ---- the staging the 128- and 256-tile kernels (and gemm_fp8.hip) pass a wave's 64 x 64 quadrant through on its way out:
// bytes per staged row (+16: rows 0/8 do not share a bank pair)
constexpr int kStagePitch = 64 * 2 + 16;

}  // namespace
