// What the LDS-staged tile GEMMs (gemm_tile128.hip, gemm_tile256.hip) share: the LDS image of an operand tile with its
// bank swizzle, its LDS-DMA staging and the fragment read that undoes the swizzle.  Beside it the host idiom of every
// launcher of the family (gemm_xs.hip and the front door gemm_f16.hip too): a run-time code or pointer becomes a
// compile-time constant argument of a lambda, and an operand list is checked for alignment by one predicate.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <stdlib.h>

#include "codetr_hip.h"
#include "device_prims.h"
#include "gemm_epilogue.h"

namespace {

constexpr int BM = 128, BN = 128;   // the 128-tile kernel's output tile (the front door bounds its tile count)
constexpr int kThreads = 256;

// f(std::integral_constant<int, ACT>) for the run-time activation code `act` (0 .. 3, checked by the callers)
template <class F>
__host__ __device__ __forceinline__ auto dispatch_act(int act, F f) {
  switch (act) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 2>{});
  }
}

// f(has_bias, has_residual) as two std::integral_constant<bool>: the four epilogue forms of a kernel (as
// persist_launch of gemm_persist.h)
template <class F>
auto dispatch_bias_res(const void* bias, const void* R, F f) {
  if (bias && R) return f(std::true_type{}, std::true_type{});
  if (bias) return f(std::true_type{}, std::false_type{});
  if (R) return f(std::false_type{}, std::true_type{});
  return f(std::false_type{}, std::false_type{});
}

// f(std::integral_constant<int, KS>): the X-stationary kernel's k-steps of 32 for K = 192 (KS 6) and K = 256 (KS 8);
// the callers have checked K
template <class F>
auto dispatch_ks(int64_t K, F f) {
  if (K == 192) return f(std::integral_constant<int, 6>{});
  return f(std::integral_constant<int, 8>{});
}

// f(T{}) for the operands' element type, an argument of the launch functions of gemm_route.h
template <class F>
auto dispatch_elem(bool bf16, F f) {
  if (bf16) return f(BFloatT{});
  return f(HalfT{});
}

// every pointer a multiple of 16 (a null pointer is)
template <class... P>
bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// a launcher's operands as the kernels take them
const unsigned short* u16(const void* p) { return static_cast<const unsigned short*>(p); }
struct Operands {
  const unsigned short *x, *w, *b, *r;
  unsigned short* y;
  const unsigned char* mk;
  Operands(const void* X, const void* W, const void* bias, const void* R, void* Y, const void* mask = nullptr)
      : x(u16(X)), w(u16(W)), b(u16(bias)), r(u16(R)), y(static_cast<unsigned short*>(Y)),
        mk(static_cast<const unsigned char*>(mask)) {}
};

// LDS image of one operand tile: [128 rows][CH = BKT/8 chunks of 16 B].  The DMA destination is lane-linear, so
// the bank swizzle lives on the SOURCE address: LDS position p of row r holds source chunk p ^ sw(r), and the
// fragment read applies the same XOR.  sw(r) spreads the 16 rows of a ds_read_b128 lane group over distinct
// 16-B slots of the 256-B bank row: (r>>1)&7 for 128-B rows, (r>>2)&3 for 64-B rows.
template <int BKT>
__device__ __forceinline__ int sw(int row) {
  // 64-byte rows: key {0, 3, 2, 1}[(row >> 2) & 3] -- the plain (row >> 2) & 3 is 2-way conflicted under ds_read_b128's
  // lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} (tests/test_lds_bank_model.py); 128-byte rows are fine as they are
  return BKT == 64 ? (row >> 1) & 7 : ((row >> 2) & 3) ^ (((row >> 2) & 1) << 1);
}

// Stage one 128 x BKT operand tile (rows row0.. of a [rows_total, K] matrix, columns k0..k0+BKT-1) into LDS with
// BKT/16 LDS-DMA instructions per thread (16 B per lane each).
template <int BKT>
__device__ __forceinline__ void stage_tile(const unsigned short* __restrict__ src, int rows_total, int K, int row0, int k0,
                                           unsigned char* lds_tile, int tid) {
  constexpr int CH = BKT / 8;
  const int wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < CH / 2; ++q) {
    const int u = q * kThreads + tid;
    const int r = u / CH, pos = u % CH;
    const int chunk = pos ^ sw<BKT>(r);
    int grow = row0 + r;
    grow = grow < rows_total ? grow : rows_total - 1;  // edge tiles: re-read the last row, results masked later
    const unsigned short* g = src + (size_t)grow * K + k0 + chunk * 8;
    // wave-uniform LDS base of this instruction; the hardware adds lane*16
    unsigned char* l = lds_tile + (q * kThreads + wave * 64) * 16;
    lds_dma16_auto(g, l);
  }
}

__device__ __forceinline__ void dma_piece(const unsigned short* g, unsigned char* lds_tile, int q, int wave) {
  unsigned char* l = lds_tile + (q * kThreads + wave * 64) * 16;
  lds_dma16_auto(g, l);
}

template <class T, int BKT>
__device__ __forceinline__ typename T::frag read_frag(const unsigned char* lds_tile, int row, int chunk) {
  const int pos = chunk ^ sw<BKT>(row);
  return *reinterpret_cast<const typename T::frag*>(lds_tile + row * (BKT * 2) + pos * 16);
}

}  // namespace
