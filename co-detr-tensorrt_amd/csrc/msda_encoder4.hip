// Encoder self-attention form of the fused multi-scale deformable attention, round-5 kernel ("v4") for MI355X (gfx950).
//
// The op: reference codetr/csrc/ms_deform_attn.cu:31-77, 211-261 plus the softmax / sampling-location steps of
// codetr/multi_scale_deformable_attention.py:180-196 and the reference points of codetr/transformer.py:280-305, for
// DetrTransformerEncoder (codetr/transformer.py:81-92: the queries ARE the pixels of the pyramid).
//
// What round 4's three-pass kernel (msda_encoder.hip, v3) spent its time on -- profiles/r03_msda_encoder_ablation.txt:
// sample preparation 34 %, per-tile skeleton 27 %, staging 20 %, the gather loop itself 18 %; ~1 300 vector instructions
// per 16 (query, head) pairs.  This kernel keeps v3's gather loop (LDS-staged per-(head, level) windows, packed-half
// blend, DPP quad hand-over, three passes over the levels) and removes the rest:
//   * LANE-MAJOR PROJECTION.  The (offsets | logits) GEMM's weight rows are permuted once on the host so that its
//     output row holds, per head, 4 x 32 bytes: the 16 halves a quad lane needs -- (x, y) of its point on the five
//     levels, its five logits, one pad.  A lane fetches its operands for an iteration with TWO 16-byte loads, a quad
//     reads one whole 128-byte line (v3: fifteen 2/4-byte loads per lane, 16 partial lines per instruction).
//   * GEOMETRY IN SCALAR REGISTERS.  Everything that depends on (image, region, head) only -- windows, LDS bases, the
//     region's query rectangles, valid pixel counts -- is wave-uniform: each wave computes it redundantly and keeps it
//     in SGPRs (no LDS table, no barriers, no per-level LDS reads inside the preparation).
//   * ZERO BORDER.  A staged window extends one pixel beyond the image where it touches the border and those cells are
//     zero-filled, so a sample needs ONE unsigned range test per axis (are its four corners staged?) and no per-corner
//     validity arithmetic: floor + fract + subtract + compare, 2 instructions for the LDS address, 9 for the weights.
//     Everything else -- samples outside the windows, outside the image, non-finite -- takes the fix-up path, which
//     re-derives the sample with the reference's full gate / corner logic and reads its rows from global memory.
//   * ROW-WISE STAGING from a head-major value map [B][M][S][32] (the value projection writes it that way): a wave takes
//     window rows, one LDS-DMA instruction moves 16 pixels of a row -- 1 KiB contiguous, 8 whole 128-byte lines -- from a
//     scalar base; 512 threads on a 16 x 16 region re-stage half as much halo per query as 256 on 16 x 8.
//   * reference points in fp32 from the valid pixel counts (as v3's CREF form): centre * vc_k / vc_q - 0.5 + offset.
// Numerics: as v3 -- fp16 corner weights (bilinear x attention), 8-term fp16 chains added into fp32 accumulators; tested
// against the fp64 oracle at the reference's half tolerance (tests/test_msda_encoder4_gpu.py).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "codetr_hip.h"
#include "device_prims.h"
#include "large_lds.h"
#include "msda_window.h"

namespace {

using namespace msda_win;

constexpr int kL = kLevels, kP = 4;
constexpr int kMaxM = 16;     // heads with a staged window of their own
constexpr int kMaxIt = 3;     // iterations (16 queries each) per wave
#ifndef MSDA4_KQ
#define MSDA4_KQ 2
#endif
constexpr int kQ = MSDA4_KQ;  // fix-up records per (query, head) pair and queue round
constexpr int kMaxLds = 160 * 1024;
#ifndef MSDA4_BAND
#define MSDA4_BAND 4
#endif
constexpr int kBand = MSDA4_BAND;   // region rows per band of the tile walk (see decode_tile; 2 / 8 measured: profiles/r05_msda_encoder4_sweep.txt)
#ifndef MSDA4_ABL
#define MSDA4_ABL 0           // timing experiments only (tools/micro/build_variant.sh): parts compiled out, WRONG results
#endif
constexpr int kAbl = MSDA4_ABL;   // 1: no wait for the staging DMA, 2: no staging, 4: no gather, 8: no preparation, 16: no barriers, 32: no output stores

#ifdef MSDA4_STAMPS   // diagnostic build only (tools/msda4_stamps.py): per-workgroup cycle stamps of wave 0
__device__ unsigned long long* g_msda4_stamps;
#define M4_T(i) const unsigned long long m4_t##i = __builtin_readcyclecounter()
#define M4_PUT(k, v) m4_s[k] = (v)
#else
#define M4_T(i)
#define M4_PUT(k, v)
#endif


struct Geom4 {
  int M, S, RX, RY;
  int H[kL], W[kL], start[kL];
  signed char win[kMaxM][kL][4];       // per (head, level): offsets (pixels of that level) in [x lo, x hi] x [y lo, y hi] are staged
  const float* vcounts;                // [B][L][2] valid pixels (w, h) of every level, fp32
  unsigned queue_off;                  // LDS byte offset of the fix-up queues (behind the largest pass)
  int head_major;                      // value map [B][M][S][32] (a head's rows contiguous) instead of [B][S][M][32]
};

// acc += (float)h.lo / (float)h.hi in one instruction each
__device__ __forceinline__ void acc_h2(float& lo, float& hi, f16x2 h) {
  const unsigned u = __builtin_bit_cast(unsigned, h);
  asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(u));
  asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(hi) : "v"(u));
}

// ET, WinF16 or WinBF16: storage type of the packed projection and of the output (the staged VALUE map is fp16 in either
// case: the blend runs on packed halves, and gfx950 has no packed bf16 FMA -- a bf16 model's value projection writes fp16,
// three mantissa bits more than bf16, through codetr_linear_bf16_f16out)

// What a wave keeps about one level (all wave-uniform: SGPRs)
struct Lv : WinLv {
  float vcx, vcy;            // valid pixels along x / y
};

template <class ET>
__device__ __forceinline__ Smp sample_at(const Lv& v, float bx, float by, unsigned o2) {
  // reference: loc = ref_k + off / (W, H); im = loc * (W, H) - 0.5 with ref_k = centre / (vr_q size_q) * vr_k and
  // vr * size = valid pixel count  ->  im = (centre / vc_q) * vc_k - 0.5 + off          (transformer.py:280-305, cu:241-247)
  return sample_of(nan_low(fmaf(bx, v.vcx, -0.5f) + ET::lo(o2)), nan_low(fmaf(by, v.vcy, -0.5f) + ET::hi(o2)));
}

template <int T>
struct Cfg {
  static constexpr int kWaves = T / 64;
  static constexpr int kPairs = T / 4;      // (query, head) pairs per workgroup iteration
};

// ---- one PASS = levels [LV0, LV0 + NLV) ---------------------------------------------------------------------------
// prepared sample: LDS address of its (x0, y0) row, the four corner weights as two packed half pairs (zero when the sample
// is not served from LDS)
struct Prep {
  unsigned ad, w01, w23;
};

template <class ET, int LV0, int NLV>
__device__ __forceinline__ bool prepare(Prep (&pp)[NLV], const Lv (&lv)[kL], const float (&aw)[kL], const unsigned (&o2)[kL],
                                        float bx, float by) {
  bool allok = true;
#pragma unroll
  for (int i = 0; i < NLV; ++i) {
    const Lv& v = lv[LV0 + i];
    const Smp s = sample_at<ET>(v, bx, by, o2[LV0 + i]);
    const WinHit h = in_window(s, v);
    const float a = aw[LV0 + i];
    const float wy1 = s.lh * a, wy0 = a - wy1, wx0 = 1.f - s.lw;
    const unsigned w01 = WinF16::pack2(wy0 * wx0, wy0 * s.lw), w23 = WinF16::pack2(wy1 * wx0, wy1 * s.lw);
    const unsigned a_in = window_addr(v, h);
    pp[i].ad = h.ok ? a_in : v.base;   // a finite staged row for the (zero-weight) reads of a sample served elsewhere
    pp[i].w01 = h.ok ? w01 : 0u;
    pp[i].w23 = h.ok ? w23 : 0u;
    allok = allok && h.ok;
  }
  return allok;
}

// gather of one iteration: 4 * NLV sample slots, one per step; rows of step s + 1 requested before the arithmetic of step s
template <int LV0, int NLV>
__device__ __forceinline__ void gather(float (&acc)[8], const Prep (&pp)[NLV], const Lv (&lv)[kL], const unsigned lds_lane) {
  using LV = const __attribute__((address_space(3))) f16x8*;
  constexpr int NS = 4 * NLV, DEPTH = 1, NB = DEPTH + 1;   // (rows two / three steps ahead measured slower: registers)
  f16x8 rows[NB][4];
  unsigned wA[NB], wB[NB];
  unsigned adr[NLV];
#pragma unroll
  for (int i = 0; i < NLV; ++i) adr[i] = pp[i].ad;
  if (NLV == 1) dpp_guard(adr[0]);   // (quad_bcast_add below reads them)
  else dpp_guard(adr[0], adr[NLV - 1]);
  auto fetch = [&](int s_, int buf) {
    const int o = s_ & 3, i = s_ >> 2;
    const unsigned a0 = quad_bcast_add(adr[i], o, lds_lane);
    const unsigned a1 = a0 + lv[LV0 + i].pitch;
    wA[buf] = quad_bcast_u(pp[i].w01, o);
    wB[buf] = quad_bcast_u(pp[i].w23, o);
    rows[buf][0] = *(LV)(uintptr_t)a0;
    rows[buf][1] = *(LV)(uintptr_t)(a0 + 64);
    rows[buf][2] = *(LV)(uintptr_t)a1;
    rows[buf][3] = *(LV)(uintptr_t)(a1 + 64);
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) fetch(d, d);
  f16x2 h[4];
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    const int b = s_ % NB;
    if (s_ + DEPTH < NS) fetch(s_ + DEPTH, (s_ + DEPTH) % NB);
    const f16x2 a = as_h2(wA[b]), c = as_h2(wB[b]);
    const f16x2 w4[4] = {f16x2{a[0], a[0]}, f16x2{a[1], a[1]}, f16x2{c[0], c[0]}, f16x2{c[1], c[1]}};
#pragma unroll
    for (int cr = 0; cr < 4; ++cr) {
      const f16x8 r = rows[b][cr];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f16x2 v = {r[2 * j], r[2 * j + 1]};
        h[j] = ((s_ & 1) == 0 && cr == 0) ? v * w4[cr] : __builtin_elementwise_fma(v, w4[cr], h[j]);
      }
    }
    if (s_ & 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc_h2(acc[2 * j], acc[2 * j + 1], h[j]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// samples the windows do not serve: re-derived with the reference's gate / corner logic (cu:52-71, 249), queued per pair
// (16-byte records in LDS), and added from global memory by the pair's four lanes, kQ records per round (requesting the
// first round's rows before the gather loop needs 20 more live registers: 91 spills at four waves per SIMD, and level at
// three -- profiles/r05_msda_encoder4_sweep.txt; not kept).
template <class ET, int LV0, int NLV>
struct Fix {
  u32x4 rec[NLV];
  unsigned bad;
  int cnt;
  f16x8 r4[kQ][4];
  u32x4 rc[kQ];

  __device__ __forceinline__ void push(u32x4* __restrict__ queue, int base, int sub) {
#pragma unroll
    for (int i = 0; i < NLV; ++i) {
      const int pt = sub + 4 * i;
      if ((bad >> pt) & 1u) {
        const int pos = __builtin_popcount(bad & ((1u << pt) - 1u)) - base;
        if ((unsigned)pos < (unsigned)kQ) queue[pos] = rec[i];
      }
    }
  }
  __device__ __forceinline__ void request(const u32x4* __restrict__ queue, int base, const unsigned char* __restrict__ vhead,
                                          unsigned pix_bytes) {
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
      if (base + j < cnt) {
        rc[j] = queue[j];
        const unsigned char* p = vhead + (size_t)rc[j][0] * pix_bytes;
        const unsigned xs = (rc[j][1] >> 16) * pix_bytes, ys = (rc[j][1] & 0xffffu) * pix_bytes;
        r4[j][0] = *reinterpret_cast<const f16x8*>(p);
        r4[j][1] = *reinterpret_cast<const f16x8*>(p + xs);
        r4[j][2] = *reinterpret_cast<const f16x8*>(p + ys);
        r4[j][3] = *reinterpret_cast<const f16x8*>(p + ys + xs);
      }
    }
  }
  __device__ __forceinline__ void blend(float (&acc)[8], int base) {
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
      if (base + j < cnt) {
        const f16x2 a = as_h2(rc[j][2]), c = as_h2(rc[j][3]);
        const f16x2 w4[4] = {f16x2{a[0], a[0]}, f16x2{a[1], a[1]}, f16x2{c[0], c[0]}, f16x2{c[1], c[1]}};
        f16x2 h[4];
#pragma unroll
        for (int cr = 0; cr < 4; ++cr)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const f16x2 v = {r4[j][cr][2 * jj], r4[j][cr][2 * jj + 1]};
            h[jj] = cr == 0 ? v * w4[cr] : __builtin_elementwise_fma(v, w4[cr], h[jj]);
          }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc_h2(acc[2 * jj], acc[2 * jj + 1], h[jj]);
      }
    }
  }

  __device__ __forceinline__ void derive(const Lv (&lv)[kL], const float (&aw)[kL], const unsigned (&o2)[kL], float bx, float by,
                                         const int sub) {
    bad = 0;
#pragma unroll
    for (int i = 0; i < NLV; ++i) {
      const Lv& v = lv[LV0 + i];
      const Smp s = sample_at<ET>(v, bx, by, o2[LV0 + i]);
      const bool ok = in_window(s, v).ok;
      const FixCorners f = fix_corners(v, s, aw[LV0 + i]);
      rec[i] = u32x4{f.first, f.strides, WinF16::pack2(f.w00, f.w01), WinF16::pack2(f.w10, f.w11)};
      bad |= (!ok && f.gate) ? 1u << (sub + 4 * i) : 0u;
    }
    bad |= dpp_u<kXor2>(bad);
    bad |= dpp_u<kXor1>(bad);
    cnt = __builtin_popcount(bad);
  }
};

// every round = queue, request, blend
template <class ET, int LV0, int NLV>
__device__ __forceinline__ void fixup(float (&acc)[8], const Lv (&lv)[kL], const float (&aw)[kL], const unsigned (&o2)[kL],
                                      float bx, float by, u32x4* __restrict__ queue, const unsigned char* __restrict__ vhead,
                                      const unsigned pix_bytes, const int sub) {
  Fix<ET, LV0, NLV> fx;
  fx.derive(lv, aw, o2, bx, by, sub);
  for (int base = 0; __builtin_amdgcn_ballot_w64(fx.cnt > base) != 0; base += kQ) {
    fx.push(queue, base, sub);
    fx.request(queue, base, vhead, pix_bytes);
    fx.blend(acc, base);
  }
}

// LDS: [staged rows of ONE pass | fix-up queues (T / 4 pairs x kQ x 16 B)]
template <class ET, int T>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(4, 4))) void msda_encoder_v4_kernel(
    const _Float16* __restrict__ value, const unsigned short* __restrict__ packed, unsigned short* __restrict__ out,
    const Geom4 g, const int packed_stride) {
  constexpr int kWaves = Cfg<T>::kWaves, kPairs = Cfg<T>::kPairs;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned lds0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)smem;

  const int tid = threadIdx.x;
  const int wave = uni(tid >> 6), lane = tid & 63, sub = lane & 3, pl = lane >> 2;
  const int M = g.M;
#ifdef MSDA4_STAMPS
  unsigned long long m4_s[20];
  for (int i = 0; i < 20; ++i) m4_s[i] = 0;
  M4_T(k0);
#endif
  // one pixel of one head = 64 bytes; consecutive pixels of a head are 64 B apart in the head-major map (a staged window
  // row is ONE contiguous run: a DMA instruction reads 8 whole 128-byte lines), M * 64 B apart in the op's own layout
  // (16 half lines per DMA instruction)
  const unsigned pix_bytes = g.head_major ? kRow : (unsigned)M * kRow;

  // ---- wave-uniform geometry -> scalar registers ----
  const TileId t0 = decode_tile<kBand>((int)xcd_tile(blockIdx.x, gridDim.x), g.M, g.RX, g.RY);
  const TileId t = {uni(t0.b), uni(t0.rx), uni(t0.ry), uni(t0.m)};
  Lv lv[kL];
  int total;
  {
    // lane 8 l + j: item j of level l (fill_levels), its window offset byte j & 3 of the (head, level)'s win word
    const int gl = lane >> 3 > kL - 1 ? kL - 1 : lane >> 3, gj = lane & 7;
    int nW = g.W[0], nH = g.H[0], wword = 0;
    const int mw = t.m < kMaxM ? t.m : kMaxM - 1;
#pragma unroll
    for (int l = 0; l < kL; ++l) {
      int ww;
      __builtin_memcpy(&ww, g.win[mw][l], 4);
      nW = gl == l ? g.W[l] : nW;
      nH = gl == l ? g.H[l] : nH;
      wword = gl == l ? ww : wword;
    }
    const int res = region_item(gj, t.rx, t.ry, nW, nH, g.RX, g.RY,
                                [&](bool) { return (int)(signed char)((unsigned)wword >> (8 * (gj & 3))); });
    total = fill_levels(lv, g.W, g.H, g.start, res, lds0);
#pragma unroll
    for (int l = 0; l < kL; ++l) {
      const float* vc = g.vcounts + ((size_t)t.b * kL + l) * 2;
      lv[l].vcx = unif(vc[0]);
      lv[l].vcy = unif(vc[1]);
    }
  }
  const int n_it = total > wave * 16 ? (total - wave * 16 + kPairs - 1) / kPairs : 0;   // <= kMaxIt (host-checked)

  const unsigned char* vhead0 = reinterpret_cast<const unsigned char*>(value) +
                                (g.head_major ? ((size_t)t.b * M + t.m) * g.S : (size_t)t.b * g.S * M + t.m) * kRow;   // (uniform)
  const unsigned char* vhead = vhead0 + sub * 16;
  const unsigned char* prow = reinterpret_cast<const unsigned char*>(packed) + (size_t)t.b * g.S * packed_stride * 2 +
                              (t.m * 64 + sub * 16) * 2;

  // ---- the wave's queries: slot -> (level, pixel) -> flattened index, centre / valid count; raw operands requested ----
  // (level_tables / slot_query; the reciprocals of the level's valid pixel counts sit in two tables of the same kind)
  const LvTables tab = level_tables(lv, lane);
  float tRx = 0.f, tRy = 0.f;
#pragma unroll
  for (int l = 0; l < kL; ++l) {
    tRx = lane == l ? lv[l].vcx : tRx;
    tRy = lane == l ? lv[l].vcy : tRy;
  }
  tRx = __builtin_amdgcn_rcpf(tRx);
  tRy = __builtin_amdgcn_rcpf(tRy);
  int qs[kMaxIt];
  float bx[kMaxIt], by[kMaxIt];
  u32x4 rawA[kMaxIt], rawB[kMaxIt];
#pragma unroll
  for (int it = 0; it < kMaxIt; ++it) {
    qs[it] = 0;
    bx[it] = by[it] = 0.f;
    rawA[it] = rawB[it] = u32x4{0u, 0u, 0u, 0u};
    if (it < n_it) {
      int sl = (it * kWaves + wave) * 16 + pl;
      sl = sl < total ? sl : total - 1;
      const SlotQuery sq = slot_query(lv, tab, sl);
      const float rx_ = __int_as_float(__builtin_amdgcn_ds_bpermute(sq.lvq, __float_as_int(tRx)));
      const float ry_ = __int_as_float(__builtin_amdgcn_ds_bpermute(sq.lvq, __float_as_int(tRy)));
      qs[it] = sq.q;
      // get_reference_points (transformer.py:280-305): centre / (valid ratio * size) = centre / valid pixel count
      bx[it] = ((float)sq.x + 0.5f) * rx_;
      by[it] = ((float)sq.y + 0.5f) * ry_;
      const unsigned char* pr = prow + (size_t)((unsigned)qs[it] * (unsigned)packed_stride) * 2;
      rawA[it] = *reinterpret_cast<const u32x4*>(pr);
      rawB[it] = *reinterpret_cast<const u32x4*>(pr + 16);
    }
  }

  // ---- softmax over the pair's 20 logits (5 per lane, quad reductions); the offsets stay packed ----
  float aw[kMaxIt][kL], acc[kMaxIt][8];
  unsigned o2[kMaxIt][kL];
#pragma unroll
  for (int it = 0; it < kMaxIt; ++it) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[it][j] = 0.f;
    o2[it][0] = rawA[it][0];
    o2[it][1] = rawA[it][1];
    o2[it][2] = rawA[it][2];
    o2[it][3] = rawA[it][3];
    o2[it][4] = rawB[it][0];
    const float lg[kL] = {ET::lo(rawB[it][1]), ET::hi(rawB[it][1]), ET::lo(rawB[it][2]), ET::hi(rawB[it][2]), ET::lo(rawB[it][3])};
    float mx = lg[0];
#pragma unroll
    for (int k = 1; k < kL; ++k) mx = fmaxf(mx, lg[k]);
    mx = fmaxf(mx, dpp_f<kXor2>(mx));
    mx = fmaxf(mx, dpp_f<kXor1>(mx));
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kL; ++k) {
      aw[it][k] = __expf(lg[k] - mx);
      sum += aw[it][k];
    }
    sum += dpp_f<kXor2>(sum);
    sum += dpp_f<kXor1>(sum);
    const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
    for (int k = 0; k < kL; ++k) aw[it][k] *= inv;
  }

  u32x4* queue = reinterpret_cast<u32x4*>(smem + g.queue_off) + (size_t)(wave * 16 + pl) * kQ;
  const unsigned lds_lane = (unsigned)sub * 16;

  auto run_pass = [&](auto lv0_c, auto nlv_c) {
    constexpr int LV0 = decltype(lv0_c)::value, NLV = decltype(nlv_c)::value;
    constexpr int PI = LV0 == 0 ? 0 : LV0 == 1 ? 1 : 2;
    (void)PI;
    M4_T(a);
    if (LV0 > 0 && !(kAbl & 16)) __syncthreads();   // every wave is done reading the previous pass's rows
    M4_T(b);
    // -- the pass's windows -> LDS
#pragma unroll
    for (int i = 0; i < NLV; ++i) stage_window<kWaves, kAbl>(lv[LV0 + i], vhead0, pix_bytes, smem, lds0, wave, lane, sub);
    M4_T(c);
    if (!(kAbl & 1)) wait_vmcnt<0>();
    M4_T(d);
    if (!(kAbl & 16)) __syncthreads();
    M4_T(e);
    // -- per iteration: addresses / weights of the pass (right in front of their gather: computed for all iterations under
    // the DMA they cost 12 more live registers and 6 spills at the 128-register budget, and measured 3-5 % slower -- the DMA's
    // latency is covered by the other workgroup of the CU either way), the gather, then the samples the windows do not serve
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it)
      if (it < n_it && !(kAbl & 4)) {
        Prep pp[NLV];
#pragma unroll
        for (int i = 0; i < NLV; ++i) pp[i] = Prep{lv[LV0 + i].base, 0u, 0u};
        bool clean = true;
        if (!(kAbl & 8)) {
          const bool ok = prepare<ET, LV0, NLV>(pp, lv, aw[it], o2[it], bx[it], by[it]);
          clean = __builtin_amdgcn_ballot_w64(!ok) == 0;
        }
        gather<LV0, NLV>(acc[it], pp, lv, lds_lane);
        if (!clean) fixup<ET, LV0, NLV>(acc[it], lv, aw[it], o2[it], bx[it], by[it], queue, vhead, pix_bytes, sub);
      }
    M4_T(f);
    // 0: barrier in front, 1: DMA issue, 2: wait for the data, 3: barrier, 4: gather + fix-up
    M4_PUT(PI * 5 + 0, m4_tb - m4_ta); M4_PUT(PI * 5 + 1, m4_tc - m4_tb); M4_PUT(PI * 5 + 2, m4_td - m4_tc);
    M4_PUT(PI * 5 + 3, m4_te - m4_td); M4_PUT(PI * 5 + 4, m4_tf - m4_te);
  };
  M4_T(k1);
  for_each_pass(run_pass);

  unsigned char* orow = reinterpret_cast<unsigned char*>(out) + ((size_t)t.b * g.S * M + t.m) * kRow + sub * 16;
#pragma unroll
  for (int it = 0; it < kMaxIt; ++it)
    if (it < n_it && (it * kWaves + wave) * 16 + pl < total)
      store_out<ET, kAbl>(orow, qs[it], M, acc[it]);   // out is [B, S, M, 32] in either case
#ifdef MSDA4_STAMPS
  M4_T(k2);
  m4_s[15] = m4_tk1 - m4_tk0;   // prologue (geometry, operand loads, softmax)
  m4_s[16] = m4_tk2 - m4_tk0;   // whole workgroup
  if (tid == 0 && g_msda4_stamps)
    for (int i = 0; i < 20; ++i) g_msda4_stamps[(size_t)blockIdx.x * 20 + i] = m4_s[i];
#endif
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct Plan4 {
  Geom4 g;
  int rc;
  int slots_cap;       // most queries any region has
  size_t lds;          // bytes per workgroup
};

inline Plan4 plan4(const int64_t* shapes, int64_t S, int M, int L, int P, const signed char* win, int region_w, int region_h,
                   int threads) {
  Plan4 pl{};
  Geom4& g = pl.g;
  pl.rc = CODETR_E_BADARG;
  if (!shapes || !win || M <= 0 || L <= 0 || P <= 0 || region_w <= 0 || region_h <= 0) return pl;
  pl.rc = CODETR_E_UNSUPPORTED;
  if (L != kL || P != kP || (threads != 256 && threads != 512)) return pl;
  g.M = M;
  g.S = (int)S;
  int64_t sum = 0;
  for (int l = 0; l < L; ++l) {
    const int64_t h = shapes[2 * l], w = shapes[2 * l + 1];
    if (h <= 0 || w <= 0 || h > 32767 || w > 32767) return pl.rc = CODETR_E_BADARG, pl;
    g.H[l] = (int)h;
    g.W[l] = (int)w;
    g.start[l] = (int)sum;
    sum += h * w;
  }
  if (sum != S) return pl.rc = CODETR_E_BADARG, pl;
  int wmax = 0;
  for (int m = 0; m < M; ++m)
    for (int l = 0; l < L; ++l) {
      const signed char* wn = win + ((size_t)m * L + l) * 4;
      if (wn[0] > wn[1] || wn[2] > wn[3]) return pl.rc = CODETR_E_BADARG, pl;
      for (int c = 0; c < 4; ++c) {
        g.win[m < kMaxM ? m : kMaxM - 1][l][c] = wn[c];
        wmax = abs(wn[c]) > wmax ? abs(wn[c]) : wmax;
      }
      if (m >= kMaxM && memcmp(wn, win + ((size_t)(kMaxM - 1) * L + l) * 4, 4) != 0) return pl;
    }
  int fine = 0;
  for (int l = 1; l < L; ++l)
    if ((int64_t)g.H[l] * g.W[l] > (int64_t)g.H[fine] * g.W[fine]) fine = l;
  g.RX = (g.W[fine] + region_w - 1) / region_w;
  g.RY = (g.H[fine] + region_h - 1) / region_h;
  for (int l = 0; l < L; ++l) {   // the kernel's reciprocal-based floor division is exact below 2^22
    if (region_dividend_bound(g.W[l], g.RX, wmax) >= (1 << 22) || region_dividend_bound(g.H[l], g.RY, wmax) >= (1 << 22)) return pl;
  }
  int rows_cap = 0, slots = 0;
  for (int m = 0; m < (M < kMaxM ? M : kMaxM); ++m) {
    int rows_pass = 0;
    slots = 0;
    for (int l = 0; l < L; ++l) {
      const signed char* wn = g.win[m][l];
      int pw = 0, ph = 0, qw = 0, qh = 0;
      for (int r = 0; r < g.RX; ++r) {
        const int lo = ext_lo(r, g.W[l], g.RX, wn[0]), hi = ext_hi(r, g.W[l], g.RX, wn[1], lo);
        const int q = q_bound(r + 1, g.W[l], g.RX) - q_bound(r, g.W[l], g.RX);
        pw = hi - lo + 1 > pw ? hi - lo + 1 : pw;
        qw = q > qw ? q : qw;
      }
      for (int r = 0; r < g.RY; ++r) {
        const int lo = ext_lo(r, g.H[l], g.RY, wn[2]), hi = ext_hi(r, g.H[l], g.RY, wn[3], lo);
        const int q = q_bound(r + 1, g.H[l], g.RY) - q_bound(r, g.H[l], g.RY);
        ph = hi - lo + 1 > ph ? hi - lo + 1 : ph;
        qh = q > qh ? q : qh;
      }
      slots += qw * qh;
      rows_pass = (pass_first(l) == l ? 0 : rows_pass) + pw * ph;
      rows_cap = rows_pass > rows_cap ? rows_pass : rows_cap;
    }
  }
  pl.slots_cap = slots;
  g.queue_off = (unsigned)rows_cap * 64u;
  pl.lds = (size_t)rows_cap * 64 + (size_t)(threads / 4) * kQ * 16;
  pl.rc = 0;
  return pl;
}

template <class ET>
int launch4(hipStream_t st, const void* value, const int64_t* shapes, const void* packed, int64_t packed_stride,
            const float* vcounts, int64_t B, int64_t S, int M, int D, int L, int P, const signed char* win, int region_w,
            int region_h, int threads, int head_major, void* out) {
  if (!value || !shapes || !packed || !vcounts || !win || !out) return CODETR_E_BADARG;
  if (B <= 0 || S <= 0 || M <= 0 || L <= 0 || P <= 0) return CODETR_E_BADARG;
  if (D != 32) return CODETR_E_UNSUPPORTED;
  if (packed_stride < (int64_t)M * 64 || (packed_stride & 7) || packed_stride > 0x7fffffff ||
      (reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(value) & 15) || (reinterpret_cast<uintptr_t>(out) & 15))
    return CODETR_E_BADARG;
  Plan4 pl = plan4(shapes, S, M, L, P, win, region_w, region_h, threads);
  if (pl.rc != 0) return pl.rc;
  if (pl.slots_cap > (threads / 4) * kMaxIt || pl.lds > (size_t)kMaxLds) return CODETR_E_UNSUPPORTED;
  if (S * M * (int64_t)64 > 0xffffffffLL || S * packed_stride * 2 > 0xffffffffLL) return CODETR_E_TOO_LARGE;   // 32-bit in-image offsets
  const int64_t blocks = B * pl.g.RX * pl.g.RY * M;
  if (blocks >= (1 << 22)) return CODETR_E_UNSUPPORTED;
  pl.g.vcounts = vcounts;
  pl.g.head_major = head_major ? 1 : 0;
  typedef void (*Kern)(const _Float16*, const unsigned short*, unsigned short*, const Geom4, const int);
  const Kern kern = threads == 512 ? msda_encoder_v4_kernel<ET, 512> : msda_encoder_v4_kernel<ET, 256>;
  if (const hipError_t e = threads == 512 ? allow_large_lds<msda_encoder_v4_kernel<ET, 512>>(kMaxLds)
                                          : allow_large_lds<msda_encoder_v4_kernel<ET, 256>>(kMaxLds);
      e != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3((unsigned)threads), pl.lds, st, static_cast<const _Float16*>(value),
                     static_cast<const unsigned short*>(packed), static_cast<unsigned short*>(out), pl.g, (int)packed_stride);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

extern "C" {

int codetr_msda_encoder_forward_packed_f16(void* stream, const void* value_dev, const int64_t* level_shapes_host,
                                           const void* packed_dev, int64_t packed_row_stride, const float* valid_counts_dev,
                                           int64_t B, int64_t S, int M, int D, int L, int P, const int8_t* windows_host,
                                           int region_w, int region_h, int threads, int value_head_major, void* out_dev) {
  return launch4<WinF16>(static_cast<hipStream_t>(stream), value_dev, level_shapes_host, packed_dev, packed_row_stride,
                       valid_counts_dev, B, S, M, D, L, P, reinterpret_cast<const signed char*>(windows_host), region_w,
                       region_h, threads, value_head_major, out_dev);
}

int codetr_msda_encoder_forward_packed_bf16(void* stream, const void* value_f16_dev, const int64_t* level_shapes_host,
                                            const void* packed_dev, int64_t packed_row_stride, const float* valid_counts_dev,
                                            int64_t B, int64_t S, int M, int D, int L, int P, const int8_t* windows_host,
                                            int region_w, int region_h, int threads, int value_head_major, void* out_dev) {
  return launch4<WinBF16>(static_cast<hipStream_t>(stream), value_f16_dev, level_shapes_host, packed_dev, packed_row_stride,
                        valid_counts_dev, B, S, M, D, L, P, reinterpret_cast<const signed char*>(windows_host), region_w,
                        region_h, threads, value_head_major, out_dev);
}

int64_t codetr_msda_encoder_packed_lds_bytes(const int64_t* level_shapes_host, int M, int L, int P, const int8_t* windows_host,
                                             int region_w, int region_h, int threads) {
  int64_t S = 0;
  if (!level_shapes_host || L != kL) return L == kL ? CODETR_E_BADARG : CODETR_E_UNSUPPORTED;
  for (int l = 0; l < L; ++l) S += level_shapes_host[2 * l] * level_shapes_host[2 * l + 1];
  const Plan4 pl = plan4(level_shapes_host, S, M, L, P, reinterpret_cast<const signed char*>(windows_host), region_w, region_h, threads);
  if (pl.rc != 0) return pl.rc;
  if (pl.slots_cap > (threads / 4) * kMaxIt) return CODETR_E_UNSUPPORTED;
  return (int64_t)pl.lds;
}

int codetr_msda_pack_projection_index(int M, int L, int P, int32_t* idx_host) {
  if (!idx_host || M <= 0) return CODETR_E_BADARG;
  if (L != kL || P != kP) return CODETR_E_UNSUPPORTED;
  const int n_off = M * L * P * 2;
  for (int m = 0; m < M; ++m)
    for (int p = 0; p < P; ++p) {
      int32_t* d = idx_host + m * 64 + p * 16;
      for (int l = 0; l < L; ++l) {
        d[2 * l] = ((m * L + l) * P + p) * 2;
        d[2 * l + 1] = ((m * L + l) * P + p) * 2 + 1;
        d[10 + l] = n_off + (m * L + l) * P + p;
      }
      d[15] = -1;
    }
  return 0;
}

#ifdef MSDA4_STAMPS
int codetr_msda4_set_stamps(void* dev_ptr) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_msda4_stamps), &dev_ptr, sizeof(dev_ptr)) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
