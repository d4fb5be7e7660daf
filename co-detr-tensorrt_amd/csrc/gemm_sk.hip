// Persistent GEMM for the large linears of the hot path (Swin stages 0-3: reference codetr/swin.py:92-112 qkv / proj,
// :331-352 the MLP):  Y[M,N] = act(X[M,K] . W[N,K]^T + bias[N]) (+ R[M,N]),  fp16 / bf16 storage, fp32 accumulation on
// v_mfma_f32_16x16x32_{f16,bf16}.  Built from what profiles/r03_gemm256_ablation.txt measured on the 256-tile kernel of
// gemm_f16.hip (a burst of fragment reads behind every barrier, the first loads of every tile exposed, 12 % tile-count
// quantisation); what each step was worth, and the forms that lost, is in profiles/r04_gemm_sk.txt.
//
//   * one 512-thread workgroup per CU, resident for the whole launch; 8 waves (two per SIMD) as 2 (m) x 4 (n), each wave
//     a 128 x 64 piece of a 256 x 256 output tile = 8 x 4 MFMA tiles, 128 accumulator registers.  (A 4-wave / 128 x 128 /
//     AGPR form of this pipeline was built first and measured 2 x slower: with one wave per SIMD nothing covers the
//     100+ cycles an LDS-DMA instruction takes to issue.)
//   * operands move global -> LDS by LDS-DMA (16 B per lane, scalar base + per-thread offset) in HALF-STAGES of 32 k:
//     W[256 rows][64 B] + X[256 rows][64 B] = 32 KiB, a ring of NS = 4 of them (5 measured the same).  In phase p a
//     wave multiplies the fragments of half-stage p (already in registers), reads those of p + 1 into the other register
//     set and issues its 4 DMA pieces of half-stage p + NS into the slot p just left; ONE counted wait + barrier per
//     phase (half-stage p + 2 has landed for everybody; everybody is done reading slot p + 1).  No MFMA ever waits for
//     an LDS read of its own phase.
//   * the half-stage stream does not stop at tile boundaries: the producer side runs NS half-stages ahead through the
//     workgroup's whole list of tiles, so the first loads of a tile fly under the previous tile's last phases and
//     epilogue (one workgroup per tile -- flag 0x20 -- measured 7-20 % slower).
//   * work list: floor(T / G) rounds of whole tiles on the G resident workgroups (XCD-aware order: the 32 workgroups of
//     an XCD walk 32 consecutive tiles, n fastest) and the T mod G left-over tiles as whole tiles of the first workgroups.
//     Stream-K (flag 0x40) cuts the left-over tiles along K into equal ranges of 64-deep k-tiles over up to G workgroups
//     (at most 4 parts per tile): a part stores its fp32 accumulators to a per-(workgroup, wave) slab and takes a ticket
//     on the tile's per-wave counter; the wave that draws the last ticket adds the other parts and runs the epilogue of
//     its piece -- no workgroup ever waits for another one (placement- and dispatch-order independent; write-through
//     slab stores + wait_vmcnt<0>() + relaxed agent atomic, the last arriver takes an agent-scope acquire;
//     MI355X_MICROARCH.md, inter-workgroup visibility).  It is correct (tools/micro/gemm_sk_bench, tests) but NOT the
//     default: at this model's K <= 3072 a 256 x 256 fp32 partial (256 KiB out, 256 KiB back in) costs as much as the
//     tile's own operand traffic, and the split measured 10-50 % slower than the quantisation it removes.
//   * MFMA roles: A = X rows, B = W rows, so a lane's accumulator column is an output column; the weight rows are staged
//     in a permuted order (on the DMA source side: tile i, column c <-> column 4 c + i of the wave's 64) so that the four
//     n-tiles give lane c the 4 consecutive output columns 4 c .. 4 c + 3 of a row: 16 adjacent lanes store one whole
//     128-byte line, 4 rows per store instruction, straight from registers -- no LDS staging (the ring keeps running).
//     Stores and residual loads are buffer instructions on a wave-uniform descriptor with ONE 32-bit lane offset and the
//     row in the scalar offset: per-lane 64-bit addresses were hoisted and spilled by the compiler, and a scratch access
//     is a vector-memory operation that waits for every LDS-DMA piece in flight (vmcnt retires in order) -- that alone
//     was 40 % of the first version's time.  For the same reason the bias sits in LDS behind the ring, and the fragments
//     of the next tile's first half-stage are dropped over the epilogue and re-read behind it (one barrier).
//
// The ring producer, the fragment offsets, the bias in LDS, the epilogue and the host-side checks are those of
// csrc/gemm_persist.h, shared with the ping-pong kernel of csrc/gemm_pp.hip.
//
// Requirements: K % 64 == 0, K >= 128, N % 8 == 0, N <= 16384, dense row-major operands, 16-byte aligned bases; M, N
// otherwise arbitrary (edge tiles clamp their loads and mask their stores).  No row mask / head-major output
// (gemm_f16.hip serves those).  The workspace (codetr_linear_sk_workspace_bytes) must be zero-filled once; every launch
// leaves its counters at zero.

// diagnostic builds only (tools/micro: -DCODETR_SK_ABL=mask gives WRONG results by construction): 1 = no LDS-DMA inside the
// main loop, 2 = no MFMAs, 4 = no fragment reads, 8 = no wait + barrier per phase, 16 = no output stores
#ifndef CODETR_SK_ABL
#define CODETR_SK_ABL 0
#endif
namespace {
constexpr int kAbl = CODETR_SK_ABL;
}

#include "gemm_persist.h"

namespace {

constexpr int kMaxParts = 4;     // stream-K: most parts a tile is cut into
constexpr int kWaves = 8;
constexpr int kSlabFloats = 8192;    // one wave's 128 x 64 fp32 accumulators

struct SkArgs : PersistArgs {
  float* slabs;        // [G][2][8 waves][8192] fp32: slab 0 = a part that starts inside its tile, slab 1 = one that starts it
  unsigned* counters;  // [stream-K tiles][8 waves]
  int D;               // tiles of the data-parallel rounds (a multiple of G); tiles D .. T-1 are the stream-K region
  int S;               // stream-K units (64-deep k-tiles): (T - D) * nk
  int Gs;              // workgroups that take part in the stream-K region (0 .. Gs-1)
  int np;              // 1: one workgroup per tile (G == T == D), XCD-aware order
};

// ---- the work list of one workgroup: stream-K range first, then the data-parallel rounds ----
struct Cursor {
  int mode;  // 0: stream-K region, 1: data-parallel rounds, 2: finished
  int u1;    // stream-K: end of this workgroup's unit range
  int r;     // data-parallel: round
  int tile, kb, ke;  // current item: tile and its range of 64-deep k-tiles
};

__device__ __forceinline__ void dp_item(Cursor& c, const SkArgs& a, int w) {
  if (c.r * a.G < a.D) {
    c.mode = 1;
    if (a.np) {   // every XCD (workgroup id mod 8) walks a contiguous run of tiles
      const int q = a.T >> 3, r = a.T & 7, x = w & 7;
      c.tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (w >> 3);
    } else {
      c.tile = (w & 7) * (a.D >> 3) + c.r * (a.G >> 3) + (w >> 3);
    }
    c.kb = 0;
    c.ke = a.nk;
  } else {
    c.mode = 2;
  }
}

__device__ __forceinline__ int sk_begin(const SkArgs& a, int w) {  // first unit of workgroup w (w <= Gs)
  return (int)((long long)w * a.S / a.Gs);
}

__device__ __forceinline__ void cursor_init(Cursor& c, const SkArgs& a, int w) {
  c.r = 0;
  c.u1 = 0;
  if (w < a.Gs) {
    const int u0 = sk_begin(a, w);
    c.u1 = sk_begin(a, w + 1);
    if (u0 < c.u1) {
      c.mode = 0;
      const int t = u0 / a.nk;
      c.tile = a.D + t;
      c.kb = u0 - t * a.nk;
      const int e = c.u1 - t * a.nk;
      c.ke = e < a.nk ? e : a.nk;
      return;
    }
  }
  dp_item(c, a, w);
}

__device__ __forceinline__ void cursor_next(Cursor& c, const SkArgs& a, int w) {
  if (c.mode == 0) {
    const int t = c.tile - a.D;
    if (t * a.nk + c.ke < c.u1) {
      c.tile++;
      c.kb = 0;
      const int e = c.u1 - (t + 1) * a.nk;
      c.ke = e < a.nk ? e : a.nk;
      return;
    }
    c.r = 0;
    dp_item(c, a, w);
    return;
  }
  if (c.mode == 1) {
    c.r++;
    dp_item(c, a, w);
  }
}

template <class T>
struct Frags {
  typename T::frag a[4];  // W rows (MFMA B operand): 4 n-tiles
  typename T::frag b[8];  // X rows (MFMA A operand): 8 m-tiles
};

template <class T, int ACT, bool HAS_BIAS, bool HAS_RES, int NS, bool SK>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void linear_sk_kernel(const SkArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[NS * kSlot + (HAS_BIAS ? kBiasBytes : 0)];   // ring, then the bias
  using frag = typename T::frag;
  constexpr int PP = 4;               // DMA pieces per wave and half-stage (2 of W, 2 of X)
  constexpr int VMN = PP * (NS - 2);  // pieces that may stay in flight at the end of a phase

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;   // 2 x 4 waves: rows wm*128, columns wn*64
  const int wg = blockIdx.x;
  const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)lds);

  Cursor cc;   // consumer side
  cursor_init(cc, a, wg);
  if (cc.mode == 2) return;   // nothing to do (fewer k-tiles in the problem than workgroups)
  Cursor pc = cc;             // producer side: NS half-stages ahead

  // ---- producer: NS half-stages ahead, through this workgroup's items and their k ranges ----
  RingProducer prod;
  prod.set_item(a, wave, lane, pc.tile, pc.kb);
  auto produce_piece = [&](int g, int slot) { prod.piece(g, slot, lds0, wave); };
  auto produce_advance = [&]() {
    if (pc.mode == 2 || prod.step(pc.ke)) return;
    cursor_next(pc, a, wg);
    if (pc.mode != 2) prod.set_item(a, wave, lane, pc.tile, pc.kb);
  };

  const unsigned offA = frag_offset(0, wn * 64, lane), offB = frag_offset(kOpBytes, wm * 128, lane);

  f32x4 acc[4][8];   // [n-tile][m-tile]
  Frags<T> F0 = {}, F1 = {};

  if (HAS_BIAS) stage_bias(lds + NS * kSlot, a.bias, a.N, tid);
  // ---- prologue: NS half-stages in flight, fragments of half-stage 0 in F0 ----
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int g = 0; g < PP; ++g) produce_piece(g, s);
    produce_advance();
  }
  wait_vmcnt<PP * (NS - 1)>();
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < 4) F0.a[j] = *reinterpret_cast<const frag*>(lds + offA + j * 1024);
    F0.b[j] = *reinterpret_cast<const frag*>(lds + offB + j * 1024);
  }
  wait_vmcnt<PP * (NS - 2)>();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  int post = 0;   // phases left in which the previous epilogue's stores may stay in flight
  int ws = 0;   // ring slot of the current half-stage p (free for the DMA of p + NS); p + 1 is read from ws + 1

  // one phase: 32 MFMAs on CUR in 4 groups of 8 (one n-tile each), 3 fragment reads of the next half-stage into NXT and
  // one DMA piece per group, then wait + barrier
#define SK_PHASE(CUR, NXT, FIRSTK)                                                                                        \
  {                                                                                                                  \
    const int rs = ws + 1 == NS ? 0 : ws + 1;                                                                        \
    const unsigned char* rbase = lds + rs * kSlot;                                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                  \
      if (!(kAbl & 4)) {                                                                                 \
        NXT.a[i] = *reinterpret_cast<const frag*>(rbase + offA + i * 1024);                                          \
        NXT.b[2 * i] = *reinterpret_cast<const frag*>(rbase + offB + (2 * i) * 1024);                                \
        NXT.b[2 * i + 1] = *reinterpret_cast<const frag*>(rbase + offB + (2 * i + 1) * 1024);                        \
      }                                                                                                              \
      if (!(kAbl & 1)) {                                                                                             \
        produce_piece(i, ws);                                                                                        \
      }                                                                                                              \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                                \
        if (kAbl & 2) asm volatile("" ::"v"(CUR.a[i]), "v"(CUR.b[j]));                                               \
        else if (FIRSTK) acc[i][j] = T::mfma(CUR.b[j], CUR.a[i], f32x4{0.f, 0.f, 0.f, 0.f});                         \
        else acc[i][j] = T::mfma(CUR.b[j], CUR.a[i], acc[i][j]);                                                     \
      }                                                                                                              \
      __builtin_amdgcn_sched_barrier(0);                                                                             \
    }                                                                                                                \
    produce_advance();                                                                                               \
    if (!(kAbl & 8)) {                                                                                               \
      /* the NS - 2 phases behind an epilogue leave its 32 output stores out of the count (vmcnt retires in order) */ \
      if (post > 0) {                                                                                                \
        wait_vmcnt<VMN + 32>();                                                                                         \
        --post;                                                                                                      \
      } else {                                                                                                       \
        wait_vmcnt<VMN>();                                                                                              \
      }                                                                                                              \
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                             \
      __builtin_amdgcn_s_barrier();                                                                                  \
    }                                                                                                                \
    ws = rs;                                                                                                         \
  }

  while (cc.mode != 2) {
    // ---- main loop of the item: 2 phases per 64-deep k-tile, the first k-tile starts the accumulators at zero ----
    SK_PHASE(F0, F1, true)
    SK_PHASE(F1, F0, false)
    for (int kk = cc.kb + 1; kk < cc.ke; ++kk) {
      SK_PHASE(F0, F1, false)
      SK_PHASE(F1, F0, false)
    }

    bool finish = true;
    if (SK && (cc.kb != 0 || cc.ke != a.nk)) {
      // ---- a part of a stream-K tile: publish the partial sums, the last arriver (per wave) continues ----
      // slab 0 of a workgroup: its part that starts inside a tile (the first item of its range); slab 1: its part that
      // starts a tile it does not finish (the last item) -- both can be pending at once
      const int t = cc.tile - a.D;
      float* slab = a.slabs + (((size_t)wg * 2 + (cc.kb == 0 ? 1 : 0)) * kWaves + wave) * kSlabFloats;
      {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(slab, 0, kSlabFloats * 4, 0x00020000);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            u32x4 v;
            __builtin_memcpy(&v, &acc[i][j], 16);
            __builtin_amdgcn_raw_buffer_store_b128(v, rs, lane * 16, (i * 8 + j) * 1024, 16 /* sc1: write-through */);
          }
      }
      wait_vmcnt<0>();   // this wave's slab has left the CU (and its L2)
      // the workgroups that hold a part of this tile: w_a .. w_b (owner of unit u = ceil((u + 1) Gs / S) - 1)
      const long long ua = (long long)t * a.nk, ub = ua + a.nk - 1;
      const int w_a = (int)(((ua + 1) * a.Gs + a.S - 1) / a.S) - 1, w_b = (int)(((ub + 1) * a.Gs + a.S - 1) / a.S) - 1;
      int parts = 0;
      for (int w2 = w_a; w2 <= w_b; ++w2) parts += sk_begin(a, w2) < sk_begin(a, w2 + 1) ? 1 : 0;
      unsigned ticket = 0;
      if (lane == 0)
        ticket = __hip_atomic_fetch_add(a.counters + t * kWaves + wave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
      finish = (int)ticket == parts - 1;
      if (finish) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        wait_vmcnt<0>();
        for (int w2 = w_a; w2 <= w_b; ++w2) {
          const int b2 = sk_begin(a, w2);
          if (w2 == wg || b2 >= sk_begin(a, w2 + 1)) continue;
          const float* other = a.slabs + (((size_t)w2 * 2 + (b2 > (int)ua ? 0 : 1)) * kWaves + wave) * kSlabFloats;
          const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(other), 0, kSlabFloats * 4, 0x00020000);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jh = 0; jh < 8; jh += 4) {   // 4 loads in flight, then their 4 adds (more spilled the accumulators)
              u32x4 v[4];
#pragma unroll
              for (int j = 0; j < 4; ++j)
                v[j] = __builtin_amdgcn_raw_buffer_load_b128(ro, lane * 16, (i * 8 + jh + j) * 1024, 0);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                f32x4 f;
                __builtin_memcpy(&f, &v[j], 16);
                acc[i][jh + j] += f;
              }
              __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (lane == 0) __hip_atomic_store(a.counters + t * kWaves + wave, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // a non-finishing stream-K part stores nothing
    const bool stored = finish && tile_epilogue<T, ACT, HAS_BIAS, HAS_RES>(acc, a, cc.tile, wm, wn, lane, lds + NS * kSlot);
    // The fragments of the next item's first half-stage (read in the last phase) are dropped over the epilogue, which needs
    // their registers (kept live, the compiler spilled around every store -- and a scratch access is a vector-memory
    // operation that waits for every LDS-DMA piece in flight).  They are read again here; the barrier keeps a wave that is
    // already in the next phase from issuing its DMA piece into that slot before everybody has re-read it.
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < 4) F0.a[j] = *reinterpret_cast<const frag*>(lds + ws * kSlot + offA + j * 1024);
      F0.b[j] = *reinterpret_cast<const frag*>(lds + ws * kSlot + offB + j * 1024);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    post = stored && !(kAbl & 16) ? NS - 2 : 0;
    cursor_next(cc, a, wg);
  }
#undef SK_PHASE
  wait_vmcnt<0>();   // the producer's redundant fetches past the end
}

// ---- host side ----
// the work list of a launch whose common fields are filled in
void sk_plan(int flags, SkArgs& a) {
  const int G = a.G, T = a.T;
  a.np = 0;
  if (flags & 0x20) {   // one workgroup per tile
    a.G = T; a.D = T; a.S = 0; a.Gs = 0; a.np = 1;
    return;
  }
  const bool no_sk = (flags & 0x40) == 0;   // stream-K split of the left-over tiles only on request (see the header)
  const int rounds = T / G;
  const int rem = T - rounds * G;
  if (no_sk && rem > 0) {   // data-parallel only (A/B): the left-over tiles are whole items of the first `rem` workgroups
    a.D = rounds * G; a.S = rem * a.nk; a.Gs = rem;
    return;
  }
  a.D = rounds * G;
  a.S = rem * a.nk;
  // workgroups of the stream-K region: every workgroup when that leaves each tile in <= kMaxParts parts, else rem * kMaxParts
  int gs = G;
  if ((int64_t)rem * kMaxParts < gs) gs = rem * kMaxParts;
  if (gs > a.S) gs = a.S;
  a.Gs = gs;
}

int64_t sk_slab_bytes(int G) { return (int64_t)G * 2 * kWaves * kSlabFloats * 4; }
int64_t sk_workspace_bytes(int G) { return sk_slab_bytes(G) + (int64_t)G * kWaves * 4; }

template <class T>
int launch_sk(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y, int64_t M, int64_t N,
              int64_t K, int act, void* ws, int64_t ws_bytes, int flags) {
  if (const int rc = persist_check(X, W, bias, R, Y, ws, M, N, K, act)) return rc;
  const int G = persist_grid();
  // the workspace is only touched by the stream-K split
  if ((flags & 0x40) && (!ws || ws_bytes < sk_workspace_bytes(G))) return CODETR_E_BADARG;
  SkArgs a;
  if (const int rc = persist_fill(a, X, W, bias, R, Y, M, N, K, G)) return rc;
  sk_plan(flags, a);
  a.slabs = static_cast<float*>(ws);
  a.counters = ws ? reinterpret_cast<unsigned*>(static_cast<unsigned char*>(ws) + sk_slab_bytes(G)) : nullptr;
  // a plan whose left-over tiles are whole items (no split) runs the instantiation without the partial-tile path
  const bool split = a.Gs > 0 && a.S != a.Gs * a.nk;
#define CODETR_SK_ACT(ACT)                                                                                              \
  return split ? persist_launch(st, a, [](auto hb, auto hr) { return &linear_sk_kernel<T, ACT, hb(), hr(), 4, true>; })  \
               : persist_launch(st, a, [](auto hb, auto hr) { return &linear_sk_kernel<T, ACT, hb(), hr(), 4, false>; })
  switch (act) {
    case 0: CODETR_SK_ACT(0);
    case 1: CODETR_SK_ACT(1);
    default: CODETR_SK_ACT(2);
  }
#undef CODETR_SK_ACT
}

}  // namespace

extern "C" {

int64_t codetr_linear_sk_workspace_bytes(void) { return sk_workspace_bytes(persist_grid()); }

int codetr_linear_sk_supported(int64_t M, int64_t N, int64_t K) { return persist_supported(M, N, K) ? 1 : 0; }

// Where the persistent kernel measured faster than the 256-tile kernel of gemm_f16.hip (tools/micro/gemm_sk_bench on the
// 4- and 8-image Swin-L shapes, profiles/r04_gemm_sk.txt): K < 1536 with at least a tile per CU: -2 ... -25 %; at K = 1536 it
// is level; the long-K
// layers (fc2 of stages 2 / 3) are level to 5 % slower and stay on the old kernel.
int codetr_linear_sk_preferred(int64_t M, int64_t N, int64_t K, int act, int has_residual) {
  (void)act;
  (void)has_residual;
  if (!persist_supported(M, N, K) || K >= 1536) return 0;
  const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
  const int64_t tn = (N + 255) / 256;
  // little of the 256-wide tile wasted (the rule of the 256-tile kernel)
  return tiles >= device_cus() && (N * 8 >= tn * 256 * 7 || (tn == 1 && N * 4 >= 256 * 3)) ? 1 : 0;
}

int codetr_linear_sk_f16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                         void* y_dev, int64_t M, int64_t N, int64_t K, int act, void* workspace_dev, int64_t workspace_bytes,
                         int flags) {
  return launch_sk<HalfT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev, M, N, K, act,
                          workspace_dev, workspace_bytes, flags);
}

int codetr_linear_sk_bf16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                          void* y_dev, int64_t M, int64_t N, int64_t K, int act, void* workspace_dev,
                          int64_t workspace_bytes, int flags) {
#if CODETR_SK_ABL
  return CODETR_E_UNSUPPORTED;   // diagnostic builds carry the fp16 instantiations only
#endif
  return launch_sk<BFloatT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev, M, N, K, act,
                            workspace_dev, workspace_bytes, flags);
}

}  // extern "C"
