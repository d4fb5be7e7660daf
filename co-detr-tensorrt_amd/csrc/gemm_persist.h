// What the two persistent 256 x 256 GEMMs (gemm_sk.hip: one barrier per phase, stream-K split; gemm_pp.hip: the two waves
// of a SIMD take turns) have in common, said once: the operand ring and its producer, the fragment offsets, the bias in
// LDS, the epilogue of a wave's 128 x 64 piece, and on the host the shape rule, the operand checks and the launch stamp.
// Each file keeps its work list, its main loop and its `preferred` rule.  The layout all of this assumes (gemm_sk.hip's
// header has the measurements behind it):
//   * 512 threads = 8 waves, a wave owns the 128 x 64 piece (m half, 64-column strip) of a tile = 8 x 4 MFMA tiles;
//   * a ring slot is one HALF-STAGE of 32 k: W[256 rows][64 B] then X[256 rows][64 B], filled by LDS-DMA (16 B per lane,
//     scalar base + per-thread offset), the 64-byte rows swizzled by key64 on the source side;
//   * MFMA roles: A = X rows, B = W rows, so a lane's accumulator column is an output column; the weight rows are staged
//     in a permuted order (tile i, column c <-> column 4 c + i of the wave's 64) so that the four n-tiles give lane c the 4
//     consecutive output columns 4 c .. 4 c + 3 of a row: 16 adjacent lanes store one whole 128-byte line.
// The including file defines `kAbl`, its diagnostic mask, first: bit 16 (no output stores) is read here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "codetr_hip.h"
#include "device_prims.h"
#include "gemm_epilogue.h"
#include "large_lds.h"

namespace {

typedef unsigned u32x2v __attribute__((__vector_size__(2 * sizeof(unsigned))));

constexpr int kSlot = 32768;     // one half-stage: W[256][64 B] then X[256][64 B]
constexpr int kOpBytes = 16384;
constexpr int kBiasBytes = 32768;     // bias in LDS: N <= 16384

// operands and problem of a launch; SkArgs / PpArgs add their work list
struct PersistArgs {
  const unsigned char* X;
  const unsigned char* W;
  const unsigned short* bias;
  const unsigned short* R;
  unsigned short* Y;
  int M, N, K;
  int tiles_n, T, nk;  // nk = K / 64
  int G;               // workgroups (a multiple of 8)
};

// swizzle key of a 64-byte LDS row (4 chunks of 16 B): {0, 3, 2, 1}[(row >> 2) & 3] -- conflict-free under
// ds_read_b128's lane groups (tests/test_lds_bank_model.py)
__device__ __forceinline__ int key64(int row) {
  const int q = (row >> 2) & 3;
  return q ^ ((q & 1) << 1);
}

// ---- producer: a wave's 2 + 2 LDS-DMA pieces of a half-stage, walking an item (a tile and a range of its 64-deep
// k-tiles) of the workgroup's work list ahead of the reads; the kernel finds the items ----
// piece P = wave + 8 q covers LDS rows P*16 .. P*16+15 (64 B each): lane -> row P*16 + (lane >> 2), position lane & 3,
// which holds source chunk (lane & 3) ^ key64(row).  W rows are permuted: LDS row q*64 + i*16 + c holds weight row
// q*64 + 4 c + i of the tile (see tile_epilogue).
struct RingProducer {
  int h;   // the next half-stage (32-deep) of the item, counted from the start of the tile's K
  const unsigned char* Wp;   // the current half-stage of the tile's W and X rows
  const unsigned char* Xp;
  // per-lane source offsets of the two pieces of each operand.  (Behind the wave-uniform members: with these in front, a
  // form of this struct that also held the item's tile had it kept in a vector register and read back with
  // v_readfirstlane at every use.)
  unsigned voffW[2], voffX[2];

  // a new item: `tile` from k-tile kb on
  __device__ __forceinline__ void set_item(const PersistArgs& a, int wave, int lane, int tile, int kb) {
    const int K = a.K, K2 = K * 2;
    const int tm = tile / a.tiles_n, tn = tile - tm * a.tiles_n;
    const int m0 = tm * 256, n0 = tn * 256;
    const int nmax = a.N - 1 - n0, mmax = a.M - 1 - m0;   // edge tiles: the last row again (its outputs are never stored)
    // (recomputed from the lane id at every tile switch: kept in registers across the main loop these constants were
    // spilled, and a scratch reload is a vector-memory operation that queues behind every LDS-DMA piece in flight)
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = (wave + 8 * q) * 16 + (ln >> 2);
      const int rw = (r & 192) + 4 * (r & 15) + ((r >> 4) & 3);
      const unsigned co = (unsigned)((((ln & 3) ^ key64(r)) * 16));
      const int rn = rw < nmax ? rw : nmax, rm = r < mmax ? r : mmax;
      voffW[q] = (unsigned)rn * (unsigned)K2 + co;
      voffX[q] = (unsigned)rm * (unsigned)K2 + co;
    }
    Wp = a.W + ((size_t)n0 * K + (size_t)kb * 64) * 2;
    Xp = a.X + ((size_t)m0 * K + (size_t)kb * 64) * 2;
    h = 2 * kb;
  }

  // one piece (g = 0, 1: W; 2, 3: X) of the current half-stage into ring slot `slot` (lds0: LDS address of the ring)
  __device__ __forceinline__ void piece(int g, int slot, unsigned lds0, int wave) const {
    const unsigned dst = lds0 + (unsigned)slot * kSlot + (unsigned)wave * 1024u;
    if (g < 2) lds_dma16(Wp, voffW[g], dst + (unsigned)g * 8192u);
    else lds_dma16(Xp, voffX[g - 2], dst + kOpBytes + (unsigned)(g - 2) * 8192u);
  }

  // on to the next half-stage of the item, whose k-tiles end at ke; false when the item is used up: the kernel then finds
  // the next one for set_item().  Past the end of its list it does neither, and the producer re-fetches its last
  // half-stage (nobody reads it): the counted waits stay uniform
  __device__ __forceinline__ bool step(int ke) {
    ++h;
    if (h >= 2 * ke) return false;
    Wp += 64;
    Xp += 64;
    return true;
  }
};

// ---- consumer: fragment i of an operand = LDS rows row0 + i*16 + (lane & 15), chunk (lane >> 4) ^ key64(row); row0 (a
// multiple of 64) is the wave's first row of the operand, which starts `op` bytes into the slot (W: 0, X: kOpBytes).
// Byte offset of fragment 0 in the slot ----
__device__ __forceinline__ unsigned frag_offset(int op, int row0, int lane) {
  const int fa = lane & 15, fc = lane >> 4;
  return (unsigned)(op + (row0 + fa) * 64 + ((fc ^ key64(fa)) * 16));
}

// the bias into LDS behind the ring (a global load in the epilogue would queue behind the DMA pieces in flight); visible to
// everybody behind the prologue's barriers
__device__ __forceinline__ void stage_bias(unsigned char* bias_lds, const unsigned short* bias, int N, int tid) {
  for (int i = tid; i * 8 < N; i += 512)
    *reinterpret_cast<u32x4*>(bias_lds + i * 16) = *reinterpret_cast<const u32x4*>(bias + i * 8);
}

// ---- epilogue of a wave's 128 x 64 piece (m half `m_half`, 64-column strip `strip`) of tile `tile`, straight from the
// accumulators ----
// Returns whether this wave issued the 32 output stores (wave-uniform: a piece wholly outside the matrix -- e.g. strips 3
// of every tile at N = 192 -- stores nothing).  The caller's relaxed wait (vmcnt(VMN + 32) in the NS - 2 phases behind an
// epilogue) is only sound behind 32 stores that were really issued: a wave without them has nothing but LDS-DMA pieces
// in its queue, and vmcnt(VMN + 32) would let it past pieces the next phases read.
template <class T, int ACT, bool HAS_BIAS, bool HAS_RES>
__device__ __forceinline__ bool tile_epilogue(f32x4 (&acc)[4][8], const PersistArgs& a, int tile, int m_half, int strip,
                                              int lane, const unsigned char* bias_lds) {
  const int fa = lane & 15;
  const int tm = tile / a.tiles_n, tn = tile - tm * a.tiles_n;
  const int m0 = tm * 256 + m_half * 128, n0 = tn * 256 + strip * 64;   // this wave's corner
  const int g = lane >> 4, nl = 4 * fa;
  const int mleft = a.M - m0, nleft = a.N - n0;   // rows / columns of the piece that exist
  const unsigned rowb = (unsigned)a.N * 2u;
  const unsigned span = (mleft > 0 && nleft > 0) ? (unsigned)(mleft < 128 ? mleft : 128) * rowb : 0u;
  // lanes whose columns do not exist get an offset outside every descriptor (loads return 0, stores are dropped)
  const unsigned voff = nl < nleft ? (unsigned)(4 * g) * rowb + (unsigned)nl * 2u : 0x80000000u;
  const int mrem = mleft - 4 * g;   // row j*16 + r of this lane exists iff j*16 + r < mrem (a constant against one register)
  // buffer descriptors on the piece's corner (wave-uniform) + ONE 32-bit lane offset; the row of a load or store goes into
  // the scalar offset.  (Per-lane 64-bit addresses were hoisted and spilled by the compiler: 32 stores, each behind a
  // scratch reload and `wait_vmcnt<0>()` -- every store waited for the one before and for the DMA pieces in flight.)
  const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(a.R)) + ((size_t)m0 * a.N + n0) * 2, 0,
      HAS_RES ? span : 0u, 0x00020000);
  uint2 rr[8][4];
  auto load_res = [&](int j0, int j1) {
#pragma unroll
    for (int j = j0; j < j1; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32x2v t2 = __builtin_amdgcn_raw_buffer_load_b64(rres, j * 16 + r < mrem ? voff : 0x80000000u,
                                                                 (unsigned)(j * 16 + r) * rowb, 0);
        rr[j][r] = uint2{t2[0], t2[1]};
      }
  };
  const bool stored = a.M > m0 && a.N > n0;
  if (stored) {
    // acc[i][j][r]: output row m0 + j*16 + 4 (lane >> 4) + r, column n0 + 4 (lane & 15) + i: the four n-tiles give the
    // lane 4 consecutive columns = 8 bytes, lanes 0-15 one 128-byte line, a store instruction 4 whole lines
    float bias4[4] = {0.f, 0.f, 0.f, 0.f};
    if (HAS_BIAS) {
      const int nb = n0 + nl < a.N ? n0 + nl : 0;
      const uint2 b2 = *reinterpret_cast<const uint2*>(bias_lds + nb * 2);
      bias4[0] = T::to_f32((unsigned short)(b2.x & 0xffffu));
      bias4[1] = T::to_f32((unsigned short)(b2.x >> 16));
      bias4[2] = T::to_f32((unsigned short)(b2.y & 0xffffu));
      bias4[3] = T::to_f32((unsigned short)(b2.y >> 16));
    }
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<unsigned char*>(a.Y) + ((size_t)m0 * a.N + n0) * 2, 0, span, 0x00020000);
    if (HAS_RES) load_res(0, 4);   // residual rows: four row sets in flight, the other four requested two row sets later
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (HAS_RES && j == 2) load_res(4, 8);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // the output rule of gemm_epilogue.h (ACT 0 .. 2, no row states), on the packed GELU
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = acc[i][j][r] + bias4[i];
        const f32x2 x01 = epi_act2<ACT, HAS_RES>(f32x2{x[0], x[1]}), x23 = epi_act2<ACT, HAS_RES>(f32x2{x[2], x[3]});
        uint2 o = {T::pack2(x01.x, x01.y), T::pack2(x23.x, x23.y)};
        if (HAS_RES) {
          // epi_residual on the four packed values (through a helper the bf16 forms compiled to other instructions):
          // fp16(fp16(linear) + residual), the two roundings of `identity + linear(x)` in the reference's fp16 path
          const uint2 q = rr[j][r];
          const float y0 = T::to_f32((unsigned short)(o.x & 0xffffu)) + T::to_f32((unsigned short)(q.x & 0xffffu));
          const float y1 = T::to_f32((unsigned short)(o.x >> 16)) + T::to_f32((unsigned short)(q.x >> 16));
          const float y2 = T::to_f32((unsigned short)(o.y & 0xffffu)) + T::to_f32((unsigned short)(q.y & 0xffffu));
          const float y3 = T::to_f32((unsigned short)(o.y >> 16)) + T::to_f32((unsigned short)(q.y >> 16));
          o = uint2{T::pack2(y0, y1), T::pack2(y2, y3)};
        }
        if (!(kAbl & 16))
          __builtin_amdgcn_raw_buffer_store_b64(u32x2v{o.x, o.y}, ry, j * 16 + r < mrem ? voff : 0x80000000u,
                                                (unsigned)(j * 16 + r) * rowb, 0);
      }
    }
  }
  return stored;
}

// ---- host side ----
// K % 64 == 0, K >= 128, N % 8 == 0, N <= 16384 (the bias in LDS), 32-bit offsets inside a tile's rows
bool persist_supported(int64_t M, int64_t N, int64_t K) {
  return M > 0 && N > 0 && K >= 128 && K % 64 == 0 && N % 8 == 0 && M <= 0x7fffffffLL && N <= 16384 &&
         255 * K * 2 + 64 < 0x7fffffffLL;
}

// null / range / alignment check of a launch's operands (ws: a workspace, or null); 0 or a CODETR_E_ code
int persist_check(const void* X, const void* W, const void* bias, const void* R, const void* Y, const void* ws, int64_t M,
                  int64_t N, int64_t K, int act) {
  if (!X || !W || !Y || M <= 0 || N <= 0 || K <= 0) return CODETR_E_BADARG;
  if (act < 0 || act > 2 || !persist_supported(M, N, K)) return CODETR_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(Y) |
       reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(ws)) & 15)
    return CODETR_E_BADARG;
  return 0;
}

// the resident grid: one workgroup per CU, a multiple of 8 (the XCD-aware tile orders)
int persist_grid() { return device_cus() / 8 * 8; }

// the common fields of a checked launch on G workgroups; 0 or a CODETR_E_ code
int persist_fill(PersistArgs& a, const void* X, const void* W, const void* bias, const void* R, void* Y, int64_t M, int64_t N,
                 int64_t K, int G) {
  const int64_t tiles_m = (M + 255) / 256, tiles_n = (N + 255) / 256, T = tiles_m * tiles_n;
  if (T > 0x3fffffff) return CODETR_E_TOO_LARGE;
  if (G <= 0) return CODETR_E_BADARG;
  a.X = static_cast<const unsigned char*>(X);
  a.W = static_cast<const unsigned char*>(W);
  a.bias = static_cast<const unsigned short*>(bias);
  a.R = static_cast<const unsigned short*>(R);
  a.Y = static_cast<unsigned short*>(Y);
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.tiles_n = (int)tiles_n; a.T = (int)T; a.nk = (int)(K / 64);
  a.G = G;
  return 0;
}

// launches the (HAS_BIAS, HAS_RES) form the operands ask for on a.G workgroups of 512 threads and returns the HIP status;
// kernel(hb, hr) names the instantiation: [](auto hb, auto hr) { return &some_kernel<..., hb(), hr(), ...>; }
template <class Args, class Kernel>
int persist_launch(hipStream_t st, const Args& a, Kernel kernel) {
  void (*k)(const Args);
  if (a.bias && a.R) k = kernel(std::true_type{}, std::true_type{});
  else if (a.bias) k = kernel(std::true_type{}, std::false_type{});
  else if (a.R) k = kernel(std::false_type{}, std::true_type{});
  else k = kernel(std::false_type{}, std::false_type{});
  hipLaunchKernelGGL(k, dim3((unsigned)a.G), dim3(512), 0, st, a);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace
