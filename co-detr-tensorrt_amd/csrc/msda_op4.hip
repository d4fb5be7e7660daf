// Windowed form of the PUBLIC multi-scale deformable attention op for MI355X (gfx950), round 6.
//
// The op: reference codetr/csrc/ms_deform_attn.cu:31-77 (bilinear sampler), 211-261 (im2col kernel), launched by :762-779
// behind torch.ops.codetr.multi_scale_deformable_attention (codetr/csrc/deformable_attention_torch.cpp:16-31):
//   out[b, q, m, :] = sum over (level l, point p) of  weight[b, q, m, l, p] * bilinear(value[b, level l, m, :], loc[b, q, m, l, p])
// with ready-made normalised sampling locations and softmax-ed weights.  The general kernel of csrc/msda_forward.hip
// (msda_tiled_kernel) gathers every corner row from global memory: 0.08 of the HBM roofline at the encoder's shape, unchanged
// for five rounds.  The model's own encoder path got its speed from csrc/msda_encoder4.hip, which needs
// the producers' cooperation (packed projection, head-major value map, windows from the offset bias).  This kernel carries
// that kernel's structure to the op's OWN operand layouts, for encoder-shaped calls (Nq == S, 5 levels x 4 points, 32-channel
// heads, fp16 or bf16 -- one template over the 16-bit element type, round 7 added the bf16 instantiation):
//   * a 512-thread workgroup serves one (16 x 16 region of the finest level, head): its queries are the pixels of the region
//     on all five levels (341 at most on a 2x pyramid); four lanes serve a (query, head) pair, lane p = point p on every level.
//   * per pass (levels {0}, {1, 2}, {3, 4}) the value rows the region's samples can reach -- the region's footprint on the level
//     grown by a margin, one extra zero-filled pixel where it touches the image border -- are staged in LDS with LDS-DMA
//     (16 pixels x the head's 64-byte slice per instruction); a sample whose four corners are staged is blended from LDS
//     (4 ds_read_b128, one unsigned range test per axis, no per-corner validity arithmetic); every other sample takes the
//     fix-up path -- the reference's full gate / corner logic, rows from global memory -- so ANY location is served exactly;
//     that query i sits at pixel i of the pyramid only decides how many samples hit their window.
//   * sampling locations and attention weights reach the lanes THROUGH LDS (north star: "sampling_locations / attention_
//     weights staged in LDS"): a pair's 80 + 40 bytes are fetched with one 16-byte and two 8-byte loads per lane (a quad reads
//     whole 16-byte pieces of the rows), written to a 144-byte record and read back transposed (lane p: its point's (x, y) on
//     the five levels, its five weights) -- 3 coalesced loads instead of the ten 2- / 4-byte ones the layout suggests.
//   * numerics as the general kernel: fp32 corner weights (bilinear x attention), every term added in fp32 -- fp16 with
//     v_fma_mix_f32 (the value read in place), bf16 widened exactly (16-bit shift / mask) and two v_fma_f32 -- one rounding
//     to nearest even at the end -- the op's tests hold it to one fp16 / bf16 ulp of the exactly rounded result
//     (tests/test_msda_gpu.py, tests/test_msda_op4_bf16_gpu.py), which the encoder kernel's packed-half chains do not meet.
//   * the pyramid's shapes are a DEVICE tensor: the grid is persistent (two workgroups per CU) and every workgroup derives
//     regions, windows and its tile list from the device-side shapes (msda_op4_plan.h); where the plan does not apply the
//     workgroups return at once and the general kernel, launched behind this one with the same plan as its skip test, serves
//     the call.
// Tested against the fp64 oracle and the reference's golden vectors through the op (tests/test_msda_gpu.py, unchanged, and
// tests/test_msda_op4_gpu.py, tests/test_msda_op4_bf16_gpu.py).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <type_traits>

#include "codetr_hip.h"
#include "device_prims.h"
#include "large_lds.h"
#include "msda_op4_plan.h"
#include "msda_window.h"

namespace {

using namespace codetr_op4;

constexpr int kQ = 1;                         // fix-up records per (query, head) pair and queue round
constexpr int kWaves = kThreads / 64;
constexpr int kRecBytes = 144;                // operand record of a pair: 128 bytes used, 144 apart (bank spread)
constexpr unsigned kWinBytes = kWinPixels * 64u;
constexpr unsigned kQueueBytes = kPairs * kQ * 32u;
constexpr unsigned kLdsBytes = kWinBytes + kQueueBytes;   // 80 896 B: two workgroups per CU
static_assert(kWaves * 16 * kRecBytes <= (int)kWinBytes, "the operand records alias the front of the window area");
#ifndef MSDA_OP4_ABL
#define MSDA_OP4_ABL 0     // timing experiments only: 2: no staging, 4: no gather, 8: no preparation, 32: no output stores (WRONG results)
#endif
constexpr int kAbl = MSDA_OP4_ABL;


// The op's two element types: the blend on top of the shared widening / rounding
struct OpF16 : WinF16 {
  // acc += (float)(half of `u`) * w in ONE instruction each: the fp16 value is read in place
  __device__ __forceinline__ static void fma2(float& lo, float& hi, unsigned u, float w) {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(u), "v"(w));
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(hi) : "v"(u), "v"(w));
  }
};
struct OpBF16 : WinBF16 {
  // gfx950 has no mixed-precision FMA that reads bf16: both halves widened, then two fp32 FMAs -- twice the fp16 blend's
  // vector instructions.  (One v_pk_fma_f32 per pair instead measured 2-5 % slower: profiles/r07_msda_op_bf16.txt)
  __device__ __forceinline__ static void fma2(float& lo, float& hi, unsigned u, float w) {
    lo = fmaf(elem(u, 0), w, lo);
    hi = fmaf(elem(u, 1), w, hi);
  }
};

// What a wave keeps about one level (all wave-uniform: SGPRs)
struct Lv : WinLv {
  float fW, fH;
};

constexpr int kBand = 4;   // region rows per band of the tile walk (decode_tile)

template <typename T>
__device__ __forceinline__ Smp sample_at(const Lv& v, unsigned o2) {
  // cu:241-247: h_im = loc_h * H - 0.5, w_im = loc_w * W - 0.5 (x first in memory)
  return sample_of(nan_low(fmaf(T::elem(o2, 0), v.fW, -0.5f)), nan_low(fmaf(T::elem(o2, 1), v.fH, -0.5f)));
}

// weight of level k out of the lane's five packed 16-bit values
template <typename T>
__device__ __forceinline__ float weight_of(const unsigned (&awp)[3], int k) { return T::elem(awp[k >> 1], k & 1); }

// prepared sample: LDS address of its (x0, y0) row, the four corner weights (zero when the sample is not served from LDS)
struct Prep {
  unsigned ad;
  float w00, w01, w10, w11;
};

// one level's sample of the lane: window test, LDS address, corner weights.  Returns false when the sample is not served
// from LDS (its weights are then zero and its address a finite staged row)
template <typename T>
__device__ __forceinline__ bool prepare(Prep& pp, const Lv& v, const float a, const unsigned o2) {
  const Smp s = sample_at<T>(v, o2);
  const WinHit h = in_window(s, v);
  const float wy1 = s.lh * a, wy0 = a - wy1, wx0 = 1.f - s.lw;
  const unsigned a_in = window_addr(v, h);
  pp.ad = h.ok ? a_in : v.base;
  pp.w00 = h.ok ? wy0 * wx0 : 0.f;
  pp.w01 = h.ok ? wy0 * s.lw : 0.f;
  pp.w10 = h.ok ? wy1 * wx0 : 0.f;
  pp.w11 = h.ok ? wy1 * s.lw : 0.f;
  return h.ok;
}

// gather of one iteration and one level: the quad's four points, one per step; the rows of step s + 1 are requested before
// the arithmetic of step s, the step's four weights broadcast when its rows are due (one level's Prep live at a time: the
// kernel runs at four waves per SIMD, 128 registers)
template <typename T>
__device__ __forceinline__ void gather_level(float (&acc)[8], const Prep& pp, const unsigned pitch, const unsigned lds_lane) {
  using LV = const __attribute__((address_space(3))) u32x4*;
  // 16 rows (4 points x 4 corners), a ring of 5 registers sets: row k + 4 is requested right before row k is consumed (a
  // double buffer of whole steps needs 8 sets: the kernel runs at four waves per SIMD, 128 registers, and spilled)
  constexpr int RING = 5;
  u32x4 rows[RING];
  unsigned adr = pp.ad;
  dpp_guard(adr);   // (quad_bcast_add below reads it)
  unsigned a0[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) a0[o] = quad_bcast_add(adr, o, lds_lane);
  auto fetch = [&](int k) {   // row k = point k >> 2, corner k & 3
    const unsigned a = a0[k >> 2] + ((k & 2) ? pitch : 0u) + ((k & 1) ? 64u : 0u);
    rows[k % RING] = *(LV)(uintptr_t)a;
  };
#pragma unroll
  for (int k = 0; k < RING - 1; ++k) fetch(k);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k + RING - 1 < 16) fetch(k + RING - 1);
    const int o = k >> 2, cr = k & 3;
    const float w = quad_bcast_f(cr == 0 ? pp.w00 : cr == 1 ? pp.w01 : cr == 2 ? pp.w10 : pp.w11, o);
#pragma unroll
    for (int j = 0; j < 4; ++j) T::fma2(acc[2 * j], acc[2 * j + 1], rows[k % RING][j], w);
    if (cr == 3) __builtin_amdgcn_sched_barrier(0);
  }
}

// samples the windows do not serve: re-derived with the reference's gate / corner logic (cu:52-71, 249), queued per pair
// (32-byte records in LDS: first pixel, corner strides, four fp32 weights) and added from global memory by the pair's four
// lanes, kQ records per round
// One sample re-derived the reference's way: (is it served by the windows?, does it pass the gate?) and its record
struct FixRec {
  u32x4 ra, rb;
  bool ok, gate;
};
template <typename T>
__device__ __forceinline__ FixRec fix_record(const Lv& v, const float a, const unsigned o2) {
  FixRec f;
  const Smp s = sample_at<T>(v, o2);
  f.ok = in_window(s, v).ok;
  const FixCorners c = fix_corners(v, s, a);
  f.gate = c.gate;
  f.ra = u32x4{c.first, c.strides, 0u, 0u};
  f.rb = u32x4{__float_as_uint(c.w00), __float_as_uint(c.w01), __float_as_uint(c.w10), __float_as_uint(c.w11)};
  return f;
}

// The rare path: one queued sample per pair and round.  Nothing but the pair's `bad` mask stays live between rounds -- the
// record of a sample is re-derived when its turn comes (the kernel runs at 128 registers; a path that kept the records and
// two rounds' rows cost the main path 27 spilled registers).
template <typename T, int LV0, int NLV>
__device__ __forceinline__ void fixup(float (&acc)[8], const Lv (&lv)[kL], const unsigned (&awp)[3], const unsigned (&o2)[kL],
                                      u32x4* __restrict__ queue, const unsigned char* __restrict__ vhead, const unsigned pix_bytes,
                                      const int sub) {
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < NLV; ++i) {
    const FixRec f = fix_record<T>(lv[LV0 + i], weight_of<T>(awp, LV0 + i), o2[LV0 + i]);
    bad |= (!f.ok && f.gate) ? 1u << (sub + 4 * i) : 0u;
  }
  bad |= dpp_u<kXor2>(bad);
  bad |= dpp_u<kXor1>(bad);
  const int cnt = __builtin_popcount(bad);
  for (int base = 0; __builtin_amdgcn_ballot_w64(cnt > base) != 0; ++base) {
#pragma unroll
    for (int i = 0; i < NLV; ++i) {
      const int pt = sub + 4 * i;
      if (((bad >> pt) & 1u) && __builtin_popcount(bad & ((1u << pt) - 1u)) == base) {
        const FixRec f = fix_record<T>(lv[LV0 + i], weight_of<T>(awp, LV0 + i), o2[LV0 + i]);
        queue[0] = f.ra;
        queue[1] = f.rb;
      }
    }
    __builtin_amdgcn_wave_barrier();   // (the quad reads what one of its lanes just queued: one wave, LDS in order -- pins the compiler)
    if (base < cnt) {
      const u32x4 rc = queue[0], wts = queue[1];
      const unsigned char* p = vhead + (size_t)rc[0] * pix_bytes;
      const unsigned xs = (rc[1] >> 16) * pix_bytes, ys = (rc[1] & 0xffffu) * pix_bytes;
      const u32x4 r0 = *reinterpret_cast<const u32x4*>(p), r1 = *reinterpret_cast<const u32x4*>(p + xs);
      const u32x4 r2 = *reinterpret_cast<const u32x4*>(p + ys), r3 = *reinterpret_cast<const u32x4*>(p + ys + xs);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        T::fma2(acc[2 * jj], acc[2 * jj + 1], r0[jj], __uint_as_float(wts[0]));
        T::fma2(acc[2 * jj], acc[2 * jj + 1], r1[jj], __uint_as_float(wts[1]));
        T::fma2(acc[2 * jj], acc[2 * jj + 1], r2[jj], __uint_as_float(wts[2]));
        T::fma2(acc[2 * jj], acc[2 * jj + 1], r3[jj], __uint_as_float(wts[3]));
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// LDS: [staged rows of ONE pass (its front doubles as the operand records) | fix-up queues]
template <typename T>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void msda_op4_kernel(
    const unsigned short* __restrict__ value, const int64_t* __restrict__ spatial_shapes, const int64_t* __restrict__ level_start,
    const unsigned short* __restrict__ loc, const unsigned short* __restrict__ weight, unsigned short* __restrict__ out,
    const int B, const int S, const int M) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned lds0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)smem;

  Plan plan;
  if (!make_plan(spatial_shapes, level_start, S, (int64_t)B * M, plan)) return;   // (uniform for the whole grid: the general kernel serves the call)
  // the plan is wave-uniform, but its integer divisions run on the vector unit: back into scalar registers, or 22 vector
  // registers stay occupied for the whole kernel (measured: 55 spills at the 128-register budget)
#pragma unroll
  for (int l = 0; l < kL; ++l) {
    plan.W[l] = uni(plan.W[l]);
    plan.H[l] = uni(plan.H[l]);
    plan.start[l] = uni(plan.start[l]);
    plan.mg[l] = uni(plan.mg[l]);
  }
  plan.RX = uni(plan.RX);
  plan.RY = uni(plan.RY);

  const int ntiles = B * plan.RX * plan.RY * M;

  // persistent tile list: the workgroups of one XCD (blockIdx & 7 under round-robin placement -- speed only) walk one
  // contiguous eighth of the tiles, 64 consecutive tiles (8 regions x 8 heads) in flight per XCD
  const int per_xcd = (int)gridDim.x >> 3, xcd = (int)blockIdx.x & 7, chunk = (ntiles + 7) >> 3;
  const int t_end = min((xcd + 1) * chunk, ntiles);

  for (int tile = xcd * chunk + ((int)blockIdx.x >> 3); tile < t_end; tile += per_xcd) {
    // Everything below is re-derived per tile from OPAQUE copies of the thread id and of the plan: left visible, the
    // compiler hoists two dozen loop-invariant values (reciprocals of the divisions, per-lane masks and offsets, float
    // copies of the level sizes) out of this loop and keeps them live across it -- 55 spills at the 128-register budget.
    int tid = threadIdx.x, Mo = M;
    asm volatile("" : "+v"(tid), "+s"(Mo));
#pragma unroll
    for (int l = 0; l < kL; ++l) asm volatile("" : "+s"(plan.W[l]), "+s"(plan.H[l]), "+s"(plan.start[l]), "+s"(plan.mg[l]));
    asm volatile("" : "+s"(plan.RX), "+s"(plan.RY));
    const int M = Mo, RX = plan.RX, RY = plan.RY;
    const int wave = uni(tid >> 6), lane = tid & 63, sub = lane & 3, pl = lane >> 2;
    const unsigned pix_bytes = (unsigned)M * kRow;   // the op's value layout [B, S, M, 32]: a head's slices are M * 64 B apart
    u32x4* const queue = reinterpret_cast<u32x4*>(smem + kWinBytes) + (size_t)(wave * 16 + pl) * kQ * 2;
    const unsigned lds_lane = (unsigned)sub * 16;
    unsigned char* const rec = smem + (wave * 16 + pl) * kRecBytes;
    // ---- wave-uniform geometry -> scalar registers ----
    const TileId t0 = decode_tile<kBand>(tile, M, RX, RY);
    const TileId t = {uni(t0.b), uni(t0.rx), uni(t0.ry), uni(t0.m)};
    Lv lv[kL];
    int total;
    {
      // lane 8 l + j: item j of level l (fill_levels), its window offset the level's margin, -mg on the low side, +mg on the high
      const int gl = lane >> 3 > kL - 1 ? kL - 1 : lane >> 3, gj = lane & 7;
      int nW = plan.W[0], nH = plan.H[0], mgl = plan.mg[0];
#pragma unroll
      for (int l = 1; l < kL; ++l) {
        nW = gl == l ? plan.W[l] : nW;
        nH = gl == l ? plan.H[l] : nH;
        mgl = gl == l ? plan.mg[l] : mgl;
      }
      const int res = region_item(gj, t.rx, t.ry, nW, nH, RX, RY, [&](bool plus) { return plus ? mgl : -mgl; });
      total = fill_levels(lv, plan.W, plan.H, plan.start, res, lds0);
#pragma unroll
      for (int l = 0; l < kL; ++l) {
        lv[l].fW = (float)plan.W[l];
        lv[l].fH = (float)plan.H[l];
      }
    }
    const int n_it = total > wave * 16 ? (total - wave * 16 + kPairs - 1) / kPairs : 0;   // <= kMaxIt (the plan's slot bound)

    const unsigned char* vhead0 = reinterpret_cast<const unsigned char*>(value) + ((size_t)t.b * S * M + t.m) * kRow;   // (uniform)
    const unsigned char* vhead = vhead0 + sub * 16;
    // the image's (query, head) pairs: pair (q, m) = q * M + m; 80 bytes of locations, 40 of weights
    const unsigned char* loc_b = reinterpret_cast<const unsigned char*>(loc) + ((size_t)t.b * S * M + t.m) * 80;
    const unsigned char* w_b = reinterpret_cast<const unsigned char*>(weight) + ((size_t)t.b * S * M + t.m) * 40;

    // ---- the wave's queries: slot -> (level, pixel) -> flattened index; raw operands requested ----
    const LvTables tab = level_tables(lv, lane);
    int qs[kMaxIt];
    u32x4 rawA[kMaxIt];
    u32x2 rawB[kMaxIt], rawC[kMaxIt];
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it) {
      qs[it] = 0;
      rawA[it] = u32x4{0u, 0u, 0u, 0u};
      rawB[it] = rawC[it] = u32x2{0u, 0u};
      if (it < n_it) {
        int sl = (it * kWaves + wave) * 16 + pl;
        sl = sl < total ? sl : total - 1;
        qs[it] = slot_query(lv, tab, sl).q;
        // a quad fetches whole 16-byte pieces of the pair's rows: lane p the four (x, y) of level p; then lane 0 level 4, lanes
        // 1 and 2 weights 0-7 / 8-15, lane 3 weights 16-19 (its second 8-byte load repeats the first: nothing past the row)
        const unsigned pair = (unsigned)qs[it] * (unsigned)M;
        const unsigned char* lp = loc_b + (size_t)pair * 80;
        const unsigned char* wp = w_b + (size_t)pair * 40;
        rawA[it] = *reinterpret_cast<const u32x4*>(lp + sub * 16);
        const unsigned char* pb = sub == 0 ? lp + 64 : wp + (sub - 1) * 16;
        rawB[it] = *reinterpret_cast<const u32x2*>(pb);
        rawC[it] = *reinterpret_cast<const u32x2*>(pb + (sub == 3 ? 0 : 8));
      }
    }

    // every wave is done with the previous tile's staged rows and queue before the records overwrite the window area
    __syncthreads();
    // ---- through LDS: the pair's record [(x, y) of level 0-4: 80 B | weights: 40 B], read back transposed ----
    float acc[kMaxIt][8];
    unsigned o2[kMaxIt][kL], awp[kMaxIt][3];   // the five weights stay packed halves (three registers per iteration)
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[it][j] = 0.f;
#pragma unroll
      for (int k = 0; k < kL; ++k) o2[it][k] = 0u;
      awp[it][0] = awp[it][1] = awp[it][2] = 0u;
      if (it < n_it) {
        *reinterpret_cast<u32x4*>(rec + sub * 16) = rawA[it];
        *reinterpret_cast<u32x2*>(rec + 64 + sub * 16) = rawB[it];
        *reinterpret_cast<u32x2*>(rec + 72 + sub * 16) = rawC[it];
        __builtin_amdgcn_wave_barrier();   // (the LDS serves one wave's operations in order; this only pins the compiler)
#pragma unroll
        for (int k = 0; k < kL; ++k) o2[it][k] = *reinterpret_cast<const unsigned*>(rec + k * 16 + sub * 4);
        unsigned short wh[kL];
#pragma unroll
        for (int k = 0; k < kL; ++k) wh[k] = *reinterpret_cast<const unsigned short*>(rec + 80 + (k * 4 + sub) * 2);
        awp[it][0] = (unsigned)wh[0] | ((unsigned)wh[1] << 16);
        awp[it][1] = (unsigned)wh[2] | ((unsigned)wh[3] << 16);
        awp[it][2] = (unsigned)wh[4];
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();   // the records are consumed: the first pass may stage over them

    auto run_pass = [&](auto lv0_c, auto nlv_c) {
      constexpr int LV0 = decltype(lv0_c)::value, NLV = decltype(nlv_c)::value;
      if (LV0 > 0) __syncthreads();   // every wave is done reading the previous pass's rows
      // -- the pass's windows -> LDS
#pragma unroll
      for (int i = 0; i < NLV; ++i) stage_window<kWaves, kAbl>(lv[LV0 + i], vhead0, pix_bytes, smem, lds0, wave, lane, sub);
      wait_vmcnt<0>();
      __syncthreads();
#pragma unroll
      for (int it = 0; it < kMaxIt; ++it)
        if (it < n_it && !(kAbl & 4)) {
          bool clean = true;
#pragma unroll
          for (int i = 0; i < NLV; ++i) {
            const Lv& v = lv[LV0 + i];
            Prep pp = Prep{v.base, 0.f, 0.f, 0.f, 0.f};
            if (!(kAbl & 8)) clean = prepare<T>(pp, v, weight_of<T>(awp[it], LV0 + i), o2[it][LV0 + i]) && clean;
            gather_level<T>(acc[it], pp, v.pitch, lds_lane);
          }
          clean = __builtin_amdgcn_ballot_w64(!clean) == 0;
          if (!clean) fixup<T, LV0, NLV>(acc[it], lv, awp[it], o2[it], queue, vhead, pix_bytes, sub);
        }
    };
    for_each_pass(run_pass);

    unsigned char* orow = reinterpret_cast<unsigned char*>(out) + ((size_t)t.b * S * M + t.m) * kRow + sub * 16;
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it)
      if (it < n_it && (it * kWaves + wave) * 16 + pl < total)
        store_out<T, kAbl>(orow, qs[it], M, acc[it]);
  }
}

template <typename T>
int op4_forward(void* stream, const void* value_dev, const int64_t* spatial_shapes_dev, const int64_t* level_start_dev,
                const void* loc_dev, const void* weight_dev, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P,
                void* out_dev) {
  if (!value_dev || !spatial_shapes_dev || !level_start_dev || !loc_dev || !weight_dev || !out_dev) return CODETR_E_BADARG;
  if (!codetr_msda_op4_supported(2, B, S, M, D, L, Nq, P)) return CODETR_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(value_dev) | reinterpret_cast<uintptr_t>(loc_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15)
    return CODETR_E_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(weight_dev) & 7) return CODETR_E_UNSUPPORTED;
  if (const hipError_t e = allow_large_lds<msda_op4_kernel<T>>((int)kLdsBytes); e != hipSuccess) return (int)e;
  const int grid = device_cus() / 8 * 8 * 2;   // two workgroups per CU, a multiple of 8
  hipLaunchKernelGGL(msda_op4_kernel<T>, dim3((unsigned)grid), dim3(kThreads), kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(value_dev), spatial_shapes_dev, level_start_dev,
                     static_cast<const unsigned short*>(loc_dev), static_cast<const unsigned short*>(weight_dev),
                     static_cast<unsigned short*>(out_dev), (int)B, (int)S, M);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

extern "C" {

int codetr_msda_op4_supported(int elem_bytes, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P) {
  // the host-visible part of the test; the device-side plan (msda_op4_plan.h) decides on the pyramid itself.  elem_bytes 2:
  // fp16 and bf16 alike
  if (elem_bytes != 2 || D != 32 || L != kL || P != kP || Nq != S || M <= 0 || B <= 0) return 0;
  if (S < 4096) return 0;                                              // a launch-bound call: the general kernel alone
  if (S * M * (int64_t)80 > 0xffffffffLL || B * S * M >= (int64_t)1 << 31) return 0;   // 32-bit in-image offsets
  return 1;
}

// Launch the windowed kernel only; the caller launches the general kernel behind it with its skip test enabled.
int codetr_msda_op4_forward_f16(void* stream, const void* value_dev, const int64_t* spatial_shapes_dev, const int64_t* level_start_dev,
                                const void* loc_dev, const void* weight_dev, int64_t B, int64_t S, int M, int D, int L, int64_t Nq,
                                int P, void* out_dev) {
  return op4_forward<OpF16>(stream, value_dev, spatial_shapes_dev, level_start_dev, loc_dev, weight_dev, B, S, M, D, L, Nq, P, out_dev);
}

int codetr_msda_op4_forward_bf16(void* stream, const void* value_dev, const int64_t* spatial_shapes_dev, const int64_t* level_start_dev,
                                 const void* loc_dev, const void* weight_dev, int64_t B, int64_t S, int M, int D, int L, int64_t Nq,
                                 int P, void* out_dev) {
  return op4_forward<OpBF16>(stream, value_dev, spatial_shapes_dev, level_start_dev, loc_dev, weight_dev, B, S, M, D, L, Nq, P, out_dev);
}

}  // extern "C"
