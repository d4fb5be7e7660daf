// Ping-pong GEMM for the long-K linears of the hot path (Swin stages 2-3: reference codetr/swin.py:92-112 qkv / proj,
// :331-352 the MLP):  Y[M,N] = act(X[M,K] . W[N,K]^T + bias[N]) (+ R[M,N]),  fp16 / bf16 storage, fp32 accumulation on
// v_mfma_f32_16x16x32_{f16,bf16}.
//
// Why a third main loop (round 6).  The ablations of the two earlier ones (profiles/r03_gemm256_ablation.txt,
// profiles/r04_gemm_sk.txt) say the same thing: the bare MFMA stream runs at the matrix pipe's ideal, and the LDS fragment
// reads (+45 %) and the LDS-DMA issue (+25 %) ADD to it instead of hiding under it.  Both kernels run the two waves of a
// SIMD through the same instruction mix at the same time (one barrier per phase keeps them in lockstep): when the LDS
// queue is full both stall, in order, in front of their MFMAs.  Here the two waves of a SIMD take turns instead
// (cdna_hip_programming.md section 5, the 8-phase template; MI355X_MICROARCH.md "Two waves per SIMD" item 9):
//
//   * 512 threads = 8 waves as 2 GROUPS (wave >> 2 = the m half of the 256 x 256 tile: one wave of each group on every
//     SIMD) x 4 (wave & 3 = a 64-column strip); a wave owns 128 x 64 outputs = 8 x 4 MFMA tiles, 128 accumulators.
//   * a phase of a wave is a LOAD segment (12 ds_read_b128 of the fragments of one 32-deep half-stage, its 4 LDS-DMA pieces
//     of a later half-stage, the counted waits) and an MFMA segment (the 32 MFMAs of that half-stage, nothing else, at
//     raised priority), each closed by a workgroup barrier.  Group 1 runs ONE barrier behind group 0, so in every interval
//     between two barriers one wave of each SIMD feeds the matrix pipe while the other one loads; no MFMA is ever issued
//     behind a memory instruction of its own wave.
//   * operands: the ring of NS = 4 half-stages and its producer of csrc/gemm_persist.h, shared with csrc/gemm_sk.hip
//     (W[256 rows][64 B] + X[256 rows][64 B] = 32 KiB per slot, LDS-DMA with a scalar base + per-thread offset, swizzle
//     on the source address), filled NS - 1 half-stages ahead of the reads; the stream does not stop at tile boundaries
//     (persistent workgroups, one per CU).
//       WAR: half-stage p is read in L(p) -- group 0 in interval 2p, group 1 in 2p + 1 -- and every wave waits for its own
//            reads (lgkmcnt(0)) BEFORE the barrier that closes its LOAD segment; slot p is refilled from L(p + 1) on
//            (interval 2p + 2 at the earliest).
//       RAW: the pieces of half-stage q are issued in L(q - NS + 1); every wave retires its own at the end of L(q - 1)
//            with vmcnt(4 (NS - 2)) (vmcnt retires in order) -- group 1 in interval 2q - 1, one barrier before the first
//            read of q (group 0, interval 2q).
//   * tile boundary: group 0 waits one barrier before its epilogue so that both groups run their epilogues together
//     (back to back they would serialise: a wave's epilogue takes ten MFMA segments), group 1 waits one barrier at the
//     start of a tile to fall behind again: 2 n + 1 barriers per tile for both (n = phases of the tile).
//   * epilogue and buffer stores: tile_epilogue of csrc/gemm_persist.h (permuted weight rows: 16 adjacent lanes write one
//     whole 128-byte line straight from the accumulators); work list: whole tiles only, as csrc/gemm_sk.hip without its
//     stream-K split.
//
// What this buys and what bounds it (profiles/r06_gemm_pp.txt, in-kernel stamps of tools/micro/pp_stamps.hip): -4 ... -10 %
// against the faster of the two older kernels on every Swin stage 2-3 shape.  Per half-stage a wave spends 505-540 cycles in
// its MFMA segment (32 x 16 + the barrier's skew), 450-520 in its LOAD segment -- 240 for the 12 fragment reads (the four
// loading waves of an interval ask the LDS for 48 KiB: 192 cycles at 256 B/clk) and ~100 for EACH of the four DMA pieces (the
// texture path takes a 1-KiB piece from each of four waves at 64 B/clk) -- and 60-190 at each barrier: 1 375 cycles per
// half-stage against 1 024 of MFMA work for the two waves of a SIMD; with the MFMAs alone the same skeleton runs at 1 118.
// Built, measured and NOT kept (tools/micro/experiments/gemm_pp_variants.hip, gemm_pp_regstage.hip): register staging
// (global_load -> VGPR -> ds_write_b128: +15 ... +25 %, the ds_write_b128 stretch the partner's MFMA segment from 512 to
// 749 cycles), a K-tile image with whole-line DMA pieces (box-dependent: -7 ... +10 %), the half-stage in two phases of 16
// MFMAs (PH = 2: level), the bias read from global memory in the epilogue (BIAS_LDS = false), one barrier per half-stage with
// the groups in opposite segment order (level), DMA-first order in the odd strips (+3 ... +6 %).
//
// Requirements: K % 64 == 0, K >= 128, N % 8 == 0, N <= 16384, dense row-major operands, 16-byte aligned bases; M, N
// otherwise arbitrary (edge tiles clamp their loads and mask their stores).  No row mask / head-major output.

// diagnostic builds only (-DCODETR_PP_ABL=mask gives WRONG results by construction): 1 = no LDS-DMA inside the main loop,
// 2 = no MFMAs, 4 = no fragment reads, 16 = no output stores
#ifndef CODETR_PP_ABL
#define CODETR_PP_ABL 0
#endif
namespace {
constexpr int kAbl = CODETR_PP_ABL;
}

#include "gemm_persist.h"

namespace {

// diagnostic build only (tools/micro/pp_stamps.hip): where every wave's cycles go -- per wave, sums over the main loops of
// [0] LOAD segment until everything is issued, [1] waiting for the staged data (vmcnt), [2] waiting for its LDS operations,
// [3] at the barrier behind the LOAD segment, [4] MFMA segment, [5] at the barrier behind it, [6] epilogue, [7] whole kernel
#ifdef CODETR_PP_STAMPS
__device__ unsigned long long* g_pp_stamps = nullptr;
#define PP_T(i) const unsigned long long pp_t##i = __builtin_readcyclecounter()
#define PP_ACC(k, a, b) pp_acc[k] += pp_t##b - pp_t##a
#define PP_STAMPS_OUT()                                                                    \
  if (lane == 0 && g_pp_stamps) {                                                          \
    pp_acc[7] = __builtin_readcyclecounter() - pp_k0;                                      \
    unsigned long long* o = g_pp_stamps + ((size_t)blockIdx.x * 8 + wave) * 8;             \
    for (int i = 0; i < 8; ++i) o[i] = pp_acc[i];                                          \
  }
#else
#define PP_T(i)
#define PP_ACC(k, a, b)
#define PP_STAMPS_OUT()
#endif

struct PpArgs : PersistArgs {
  int rounds;          // whole rounds of G tiles
  int rem;             // T - rounds * G left-over tiles: one more item of workgroups 0 .. rem-1 (taken first)
};

// a workgroup barrier that nothing is scheduled across (MFMAs are register-only: the scheduler would otherwise move them
// past the barrier into the other group's segment)
__device__ __forceinline__ void seg_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// tile of item `idx` of workgroup w, -1 past the end.  Left-over tiles first (whole items of workgroups 0 .. rem-1), then
// the rounds: the 32 workgroups of an XCD (w mod 8) walk consecutive tiles, n fastest.
__device__ __forceinline__ int item_tile(const PpArgs& a, int w, int idx) {
  const int D = a.rounds * a.G;
  if (w < a.rem) {
    if (idx == 0) return D + w;
    --idx;
  }
  if (idx >= a.rounds) return -1;
  return (w & 7) * (D >> 3) + idx * (a.G >> 3) + (w >> 3);
}

template <class T, int ACT, bool HAS_BIAS, bool HAS_RES, int NS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void linear_pp_kernel(const PpArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[NS * kSlot + (HAS_BIAS ? kBiasBytes : 0)];   // ring, then the bias
  using frag = typename T::frag;
  constexpr int PP = 4;               // DMA pieces per wave and half-stage (2 of W, 2 of X)
  constexpr int VMN = PP * (NS - 2);  // pieces that may stay in flight at the end of a LOAD segment

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, wn = wave & 3;   // group = m half (rows grp*128), strip = columns wn*64
  const int wg = blockIdx.x;
  const int nh = 2 * a.nk;                    // half-stages (phases) of a tile
  const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)lds);

#ifdef CODETR_PP_STAMPS
  unsigned long long pp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long pp_k0 = __builtin_readcyclecounter();
#endif
  int c_idx = 0;
  int c_tile = item_tile(a, wg, 0);
  if (c_tile < 0) return;   // nothing to do (wave-uniform for the whole workgroup: no barrier has been executed)

  // ---- producer: NS - 1 half-stages ahead of the reads, whole tiles (k-tiles 0 .. nk) ----
  RingProducer prod;
  int p_idx = 0, p_tile = c_tile;   // producer's item, its tile (-1: past the end)
  prod.set_item(a, wave, lane, p_tile, 0);
  auto produce_piece = [&](int g, int slot) { prod.piece(g, slot, lds0, wave); };
  auto produce_advance = [&]() {
    if (p_tile < 0 || prod.step(a.nk)) return;
    p_tile = item_tile(a, wg, ++p_idx);
    if (p_tile >= 0) prod.set_item(a, wave, lane, p_tile, 0);
  };

  const unsigned offA = frag_offset(0, wn * 64, lane), offB = frag_offset(kOpBytes, grp * 128, lane);

  f32x4 acc[4][8];   // [n-tile][m-tile]
  frag fw[4], fx[8]; // W rows (MFMA B operand): 4 n-tiles; X rows (MFMA A operand): 8 m-tiles

  if (HAS_BIAS) stage_bias(lds + NS * kSlot, a.bias, a.N, tid);
  // ---- prologue: half-stages 0 .. NS-2 in flight, half-stage 0 landed for everybody ----
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) {
#pragma unroll
    for (int g = 0; g < PP; ++g) produce_piece(g, s);
    produce_advance();
  }
  wait_vmcnt<VMN>();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the bias rows written above
  seg_barrier();
  int post = 0;   // LOAD segments left in which the previous epilogue's stores may stay in flight
  int ws = 0;     // ring slot of the current half-stage p; slot ws - 1 is free for the DMA of p + NS - 1

  // LOAD segment: the fragment reads of half-stage p, the PP pieces of half-stage p + NS - 1 into the slot p - 1 left, and
  // the counted wait that retires half-stage p + 1; every wave waits for its own reads before it arrives at the barrier.
  auto load_seg = [&]() {
    PP_T(0);
    const unsigned char* rbase = lds + ws * kSlot;
    const int fs = ws == 0 ? NS - 1 : ws - 1;
    if (!(kAbl & 4)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) fw[i] = *reinterpret_cast<const frag*>(rbase + offA + i * 1024);
#pragma unroll
      for (int j = 0; j < 8; ++j) fx[j] = *reinterpret_cast<const frag*>(rbase + offB + j * 1024);
    }
    if (!(kAbl & 1)) {
#pragma unroll
      for (int g = 0; g < PP; ++g) produce_piece(g, fs);
    }
    produce_advance();
    PP_T(1);
    // the NS - 2 LOAD segments behind an epilogue leave its 32 output stores out of the count (vmcnt retires in order)
    if (post > 0) {
      wait_vmcnt<VMN + 32>();
      --post;
    } else {
      wait_vmcnt<VMN>();
    }
    PP_T(2);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PP_T(3);
    seg_barrier();
    PP_T(4);
    PP_ACC(0, 0, 1); PP_ACC(1, 1, 2); PP_ACC(2, 2, 3); PP_ACC(3, 3, 4);
  };
  // MFMA segment
  auto mfma_seg = [&](bool firstk) {
    PP_T(5);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (kAbl & 2) asm volatile("" ::"v"(fw[i]), "v"(fx[j]));
        else if (firstk) acc[i][j] = T::mfma(fx[j], fw[i], f32x4{0.f, 0.f, 0.f, 0.f});
        else acc[i][j] = T::mfma(fx[j], fw[i], acc[i][j]);
      }
    __builtin_amdgcn_s_setprio(0);
    PP_T(6);
    seg_barrier();
    PP_T(7);
    PP_ACC(4, 5, 6); PP_ACC(5, 6, 7);
  };

  while (c_tile >= 0) {
    if (grp == 1) seg_barrier();   // group 1 falls one barrier behind
    // ---- main loop of the tile: the first half-stage starts the accumulators at zero ----
    load_seg();
    mfma_seg(true);
    ws = ws + 1 == NS ? 0 : ws + 1;
    for (int h = 1; h < nh; ++h) {
      load_seg();
      mfma_seg(false);
      ws = ws + 1 == NS ? 0 : ws + 1;
    }
    if (grp == 0) seg_barrier();   // group 0 waits for group 1's last MFMA segment: both epilogues run together

    PP_T(8);
    const bool stored = tile_epilogue<T, ACT, HAS_BIAS, HAS_RES>(acc, a, c_tile, grp, wn, lane, lds + NS * kSlot);
    PP_T(9);
    PP_ACC(6, 8, 9);
    post = stored && !(kAbl & 16) ? NS - 2 : 0;
    c_tile = item_tile(a, wg, ++c_idx);
  }
  wait_vmcnt<0>();   // the producer's redundant fetches past the end
  PP_STAMPS_OUT();
}

// ---- host side ----
template <class T>
int launch_pp(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y, int64_t M, int64_t N,
              int64_t K, int act, int flags) {
  if (const int rc = persist_check(X, W, bias, R, Y, nullptr, M, N, K, act)) return rc;
  PpArgs a;
  if (const int rc = persist_fill(a, X, W, bias, R, Y, M, N, K, persist_grid())) return rc;
  a.rounds = a.T / a.G;
  a.rem = a.T - a.rounds * a.G;
  if ((int64_t)256 * K * 2 > 0x7fffffffLL) return CODETR_E_TOO_LARGE;   // 32-bit offsets inside a tile's rows
  if (flags != 0) return CODETR_E_UNSUPPORTED;   // (the measured variants live in tools/micro/experiments/gemm_pp_variants.hip)
  switch (act) {
    case 0: return persist_launch(st, a, [](auto hb, auto hr) { return &linear_pp_kernel<T, 0, hb(), hr(), 4>; });
    case 1: return persist_launch(st, a, [](auto hb, auto hr) { return &linear_pp_kernel<T, 1, hb(), hr(), 4>; });
    default: return persist_launch(st, a, [](auto hb, auto hr) { return &linear_pp_kernel<T, 2, hb(), hr(), 4>; });
  }
}

}  // namespace

extern "C" {

int codetr_linear_pp_supported(int64_t M, int64_t N, int64_t K) { return persist_supported(M, N, K) ? 1 : 0; }

// Where the ping-pong kernel measured faster than both older kernels (tools/micro/gemm_sk_bench on the 4- and 8-image Swin-L
// shapes over three boxes, profiles/r06_gemm_pp.txt): K >= 768 on problems of at least 200 tiles that waste little of a
// 256-wide tile -- every linear of Swin stages 2 and 3 and stage 1's fc2 (-4 ... -10 %).  The K = 384 layers are level (stay on
// the persistent kernel), N = 192 (stage 0's fc2) is 3 % behind.
int codetr_linear_pp_preferred(int64_t M, int64_t N, int64_t K, int act, int has_residual) {
  (void)act;
  (void)has_residual;
  if (!persist_supported(M, N, K) || K < 768 || N < 384) return 0;
  const int64_t tn = (N + 255) / 256, tiles = ((M + 255) / 256) * tn;
  return tiles >= 200 && N * 8 >= tn * 256 * 7 ? 1 : 0;
}

int codetr_linear_pp_f16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                         void* y_dev, int64_t M, int64_t N, int64_t K, int act, int flags) {
  return launch_pp<HalfT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev, M, N, K, act, flags);
}

int codetr_linear_pp_bf16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                          void* y_dev, int64_t M, int64_t N, int64_t K, int act, int flags) {
#if CODETR_PP_ABL
  return CODETR_E_UNSUPPORTED;   // diagnostic builds carry the fp16 instantiations only
#endif
  return launch_pp<BFloatT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev, M, N, K, act, flags);
}

}  // extern "C"
