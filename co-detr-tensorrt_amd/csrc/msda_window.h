// What the two windowed MSDA kernels share on the device (csrc/msda_encoder4.hip: the model's packed encoder kernel;
// csrc/msda_op4.hip: the windowed form of the public op): a (region, head) tile's wave-uniform geometry, the slot -> query
// lookup, the sample / window test, the reference's corner rule of the fix-up path, the row-wise LDS-DMA staging of a
// window, the DPP-hazard guard and the output store.  What differs stays with the kernels: where operands come from, the
// blend numerics, the window offsets, the fix-up queue protocol, planning and launch.
//
// Everything is __device__ __forceinline__ and sits in the anonymous namespace of the including kernel source (as
// device_prims.h).  A diagnostic build's ablation mask reaches a shared function as a template argument; nothing here reads
// a macro.
#pragma once
#include <type_traits>

#include "device_prims.h"
#include "msda_window_geom.h"

namespace {

using msda_win::kLevels;

constexpr unsigned kRow = 64;   // bytes of one pixel of one head: 32 channels of a 16-bit type

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float unif(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__device__ __forceinline__ f16x2 as_h2(unsigned u) { return __builtin_bit_cast(f16x2, u); }

// The two 16-bit element types, as (low, high) element pairs of a dword.  Both are 2 bytes wide: staging, operand layout,
// geometry and fix-up queue do not depend on which; only widening, the blend and the final rounding do.
struct WinF16 {
  __device__ __forceinline__ static float lo(unsigned u) { return (float)as_h2(u)[0]; }
  __device__ __forceinline__ static float hi(unsigned u) { return (float)as_h2(u)[1]; }
  __device__ __forceinline__ static float elem(unsigned u, int i) { return (float)as_h2(u)[i]; }
  __device__ __forceinline__ static unsigned pack2(float a, float b) {   // v_cvt_pk_f16_f32 (round to nearest even)
    const f16x2 v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(unsigned, v);
  }
};
struct WinBF16 {
  // exact widening: a bf16 value is the top half of the fp32 one (one shift / one mask)
  __device__ __forceinline__ static float lo(unsigned u) { return bf16_to_f32((unsigned short)u); }
  __device__ __forceinline__ static float hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
  __device__ __forceinline__ static float elem(unsigned u, int i) { return i ? hi(u) : lo(u); }
  __device__ __forceinline__ static unsigned pack2(float a, float b) {   // v_cvt_pk_bf16_f32 (round to nearest even; a NaN stays a NaN)
    const bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, v);
  }
};

// ---- tiles ---------------------------------------------------------------------------------------------------------
struct TileId {
  int b, rx, ry, m;
};
// tile -> (image, region column / row, head): heads innermost (the M slices of a 512-byte pixel row meet in one XCD's L2),
// regions in horizontal bands of kBand rows walked column by column (vertically adjacent regions share most of their
// windows: an L2 hit instead of a second trip over the fabric)
template <int kBand>
__device__ __forceinline__ TileId decode_tile(int tile, int M, int RX, int RY) {
  using msda_win::idiv;
  TileId t;
  const int unit = idiv(tile, M);
  t.m = tile - unit * M;
  const int regions = RX * RY;
  t.b = idiv(unit, regions);
  const int reg = unit - t.b * regions;
  const int per_band = kBand * RX;
  const int band = idiv(reg, per_band);
  const int r = reg - band * per_band;
  const int y0 = band * kBand;
  const int bh = min(kBand, RY - y0);
  t.rx = idiv(r, bh);
  t.ry = y0 + (r - t.rx * bh);
  return t;
}

// ---- levels --------------------------------------------------------------------------------------------------------
// What a wave keeps about one level (all wave-uniform: SGPRs).  Each kernel adds its own two floats.
struct WinLv {
  int W, H, start;           // level size, first pixel inside S
  int px0, py0;              // window origin, extended coordinates (-1 / size = the zero border)
  int xspan, yspan;          // largest (x0 - px0), (y0 - py0) whose four corners are staged
  int pw, ph;                // staged columns / rows
  unsigned base;             // LDS byte address of staged pixel (px0, py0)
  unsigned pitch;            // pw * 64
  int qx0, qy0, qw, slot0;   // the region's queries on this level: rectangle origin, width, first slot
};

// The tile's geometry costs 40 divisions (per level: two window bounds and two query bounds per axis), one per LANE: lane
// 8 l + j computes msda_win::region_item j of level l into `res` -- 0: first staged column, 1: last staged column (before
// the "at least two columns" clamp), 2 / 3: rows, 4 / 5: first query column of this region / of the next, 6 / 7: rows -- and
// the results return to scalar registers here, with v_readlane.  (Computed level by level in wave-uniform code this was
// 600 vector instructions per wave, a fifth of the encoder kernel.)  Fills the common part of lv[] -- windows, the LDS base
// of each inside its pass's buffer, the query rectangles and their slot prefix -- and returns the region's query count.
template <class LvT>
__device__ __forceinline__ int fill_levels(LvT (&lv)[kLevels], const int (&W)[kLevels], const int (&H)[kLevels],
                                           const int (&start)[kLevels], const int res, const unsigned lds0) {
  int slot = 0;
  unsigned base = lds0;
#pragma unroll
  for (int l = 0; l < kLevels; ++l) {
    LvT& v = lv[l];
    v.W = W[l];
    v.H = H[l];
    v.start = start[l];
    v.px0 = __builtin_amdgcn_readlane(res, 8 * l + 0);
    int px1 = __builtin_amdgcn_readlane(res, 8 * l + 1);
    v.py0 = __builtin_amdgcn_readlane(res, 8 * l + 2);
    int py1 = __builtin_amdgcn_readlane(res, 8 * l + 3);
    px1 = px1 < v.px0 + 1 ? v.px0 + 1 : px1;
    py1 = py1 < v.py0 + 1 ? v.py0 + 1 : py1;
    v.pw = px1 - v.px0 + 1;
    v.ph = py1 - v.py0 + 1;
    v.xspan = v.pw - 2;
    v.yspan = v.ph - 2;
    v.pitch = (unsigned)v.pw * kRow;
    if (msda_win::pass_first(l) == l) base = lds0;       // a new pass starts at the front of the buffer
    v.base = base;
    base += (unsigned)(v.pw * v.ph) * kRow;
    v.qx0 = __builtin_amdgcn_readlane(res, 8 * l + 4);
    v.qy0 = __builtin_amdgcn_readlane(res, 8 * l + 6);
    v.qw = __builtin_amdgcn_readlane(res, 8 * l + 5) - v.qx0;
    const int qh = __builtin_amdgcn_readlane(res, 8 * l + 7) - v.qy0;
    v.slot0 = slot;
    slot += v.qw * qh;
  }
  return slot;
}

// the passes, in order: f(first level, number of levels) as integral constants
template <class F>
__device__ __forceinline__ void for_each_pass(F&& f) {
  static_assert(msda_win::pass_first(0) == 0 && msda_win::pass_first(2) == 1 && msda_win::pass_first(4) == 3, "passes {0}, {1, 2}, {3, 4}");
  f(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
  f(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
  f(std::integral_constant<int, 3>{}, std::integral_constant<int, 2>{});
}

// ---- slot -> query -------------------------------------------------------------------------------------------------
// Per-level tables, level l in LANE l (a select between two scalars costs two vector instructions -- one constant-bus
// operand per instruction -- so a per-lane level lookup is a ds_bpermute from these instead of a select chain)
struct LvTables {
  int s0, a, b, st;
};
template <class LvT>
__device__ __forceinline__ LvTables level_tables(const LvT (&lv)[kLevels], const int lane) {
  LvTables t = {0, 0, 0, 0};
#pragma unroll
  for (int l = 0; l < kLevels; ++l) {
    const bool me = lane == l;
    t.s0 = me ? lv[l].slot0 : t.s0;
    t.a = me ? (lv[l].qx0 | (lv[l].qy0 << 16)) : t.a;
    t.b = me ? (lv[l].W | (lv[l].qw << 16)) : t.b;
    t.st = me ? lv[l].start : t.st;
  }
  return t;
}
// slot of the region -> its level (as the byte address of the level's lane, for the kernel's own ds_bpermute lookups),
// pixel and flattened query index
struct SlotQuery {
  int lvq, x, y, q;
};
template <class LvT>
__device__ __forceinline__ SlotQuery slot_query(const LvT (&lv)[kLevels], const LvTables& t, const int sl) {
  SlotQuery r;
  r.lvq = 0;
#pragma unroll
  for (int l = 1; l < kLevels; ++l) r.lvq += sl >= lv[l].slot0 ? 4 : 0;
  const int s0 = __builtin_amdgcn_ds_bpermute(r.lvq, t.s0), cA = __builtin_amdgcn_ds_bpermute(r.lvq, t.a);
  const int cB = __builtin_amdgcn_ds_bpermute(r.lvq, t.b), st = __builtin_amdgcn_ds_bpermute(r.lvq, t.st);
  const int tq = sl - s0, qw = cB >> 16, W = cB & 0xffff;
  const int yy = (int)(((float)tq + 0.5f) * __builtin_amdgcn_rcpf((float)qw));
  r.y = (cA >> 16) + yy;
  r.x = (cA & 0xffff) + (tq - yy * qw);
  r.q = st + r.y * W + r.x;
  return r;
}

// ---- samples -------------------------------------------------------------------------------------------------------
// one sample of the lane (level k, the lane's point): image coordinates -> (floor, fraction)
struct Smp {
  float lw, lh;
  int x0, y0;
};
// a NaN coordinate becomes a huge negative one -> outside every window and outside the gate: the sample is dropped, as by
// the reference's comparisons
__device__ __forceinline__ float nan_low(const float im) { return fmaxf(im, -3.0e38f); }
__device__ __forceinline__ Smp sample_of(const float w_im, const float h_im) {
  Smp s;
  s.lw = __builtin_amdgcn_fractf(w_im);
  s.lh = __builtin_amdgcn_fractf(h_im);
  s.x0 = floor_i(w_im);
  s.y0 = floor_i(h_im);
  return s;
}
// Are all four corners of the sample staged (or zero border)?  A staged window extends one pixel beyond the image where it
// touches the border and those cells are zero-filled, so ONE unsigned range test per axis decides, and a sample that passes
// needs no per-corner validity arithmetic.
struct WinHit {
  bool ok;
  unsigned dx, dy;
};
__device__ __forceinline__ WinHit in_window(const Smp& s, const WinLv& v) {
  WinHit h;
  h.dx = (unsigned)(s.x0 - v.px0);
  h.dy = (unsigned)(s.y0 - v.py0);
  h.ok = h.dx <= (unsigned)v.xspan && h.dy <= (unsigned)v.yspan;
  return h;
}
// LDS byte address of the sample's (x0, y0) pixel
__device__ __forceinline__ unsigned window_addr(const WinLv& v, const WinHit& h) { return __umul24(h.dy, v.pitch) + v.base + (h.dx << 6); }

// The fix-up path's sample, the reference's way (cu:52-71, 249): the gate, the first two words of its queue record -- first
// pixel inside S, then (row stride | column stride << 16) between the clamped corners, in pixels -- and the four corner
// weights (bilinear x attention weight a), zero for a corner outside the image.
struct FixCorners {
  bool gate;
  unsigned first, strides;
  float w00, w01, w10, w11;
};
__device__ __forceinline__ FixCorners fix_corners(const WinLv& v, const Smp& s, const float& a) {
  FixCorners f;
  // cu:249: h_im > -1 && w_im > -1 && h_im < H && w_im < W  <=>  floor in [-1, size - 1]
  f.gate = (unsigned)(s.x0 + 1) <= (unsigned)v.W && (unsigned)(s.y0 + 1) <= (unsigned)v.H;
  const float wy0 = s.y0 >= 0 ? (1.f - s.lh) * a : 0.f, wy1 = s.y0 + 1 <= v.H - 1 ? s.lh * a : 0.f;   // cu:52-71
  const float wx0 = s.x0 >= 0 ? 1.f - s.lw : 0.f, wx1 = s.x0 + 1 <= v.W - 1 ? s.lw : 0.f;
  const int x0c = max(s.x0, 0), x1c = min(s.x0 + 1, v.W - 1), y0c = max(s.y0, 0), y1c = min(s.y0 + 1, v.H - 1);
  f.first = (unsigned)(v.start + y0c * v.W + x0c);
  f.strides = (unsigned)((y1c - y0c) * v.W) | ((unsigned)(x1c - x0c) << 16);
  f.w00 = wy0 * wx0;
  f.w01 = wy0 * wx1;
  f.w10 = wy1 * wx0;
  f.w11 = wy1 * wx1;
  return f;
}

// ---- staging -------------------------------------------------------------------------------------------------------
// One level's window -> LDS, ROW-WISE: a wave takes window rows y = wave, wave + kWaves, ...; one LDS-DMA instruction moves
// 16 pixels of the row (4 lanes x 16 B per pixel = its 64-byte head slice) from a wave-uniform 64-bit base in SGPRs + a
// per-lane constant offset to the uniform LDS address of the row's chunk (+ 16 B per lane): no per-lane row / column
// arithmetic (the piece-linear walk of rounds 2-4 spent ~14 vector instructions per DMA on a division).  Cells outside the
// image -- the zero border -- are written by ds_write instead.  vhead0: the head's slice of pixel 0 of the image;
// pix_bytes: distance of consecutive pixels of a head.  The caller waits (wait_vmcnt<0>) and synchronises.  kAbl & 2: no
// staging (timing experiments).  The operands come by reference, as the kernels' pass lambdas capture them: by value the
// same loops compiled to another schedule (profiles/r23_msda_window.txt); store_out and fix_corners likewise.
template <int kWaves, int kAbl>
__device__ __forceinline__ void stage_window(const WinLv& v, const unsigned char* const& vhead0, const unsigned& pix_bytes,
                                             unsigned char* const& smem, const unsigned& lds0, const int& wave, const int& lane,
                                             const int& sub) {
  const int px_l = lane >> 2;                                      // pixel of the chunk this lane serves
  const unsigned voff = (unsigned)px_l * pix_bytes + (unsigned)sub * 16;
  const int chunks = (v.pw + 15) >> 4;
  for (int y = wave; y < ((kAbl & 2) ? 0 : v.ph); y += kWaves) {
    const int gy = v.py0 + y;
    const bool row_in = (unsigned)gy < (unsigned)v.H;              // (uniform)
    for (int c = 0; c < chunks; ++c) {
      const int x0 = 16 * c;                                       // window column of lane 0's pixel
      const unsigned dst = (v.base - lds0) + (unsigned)(y * v.pw + x0) * kRow;
      const int gx = v.px0 + x0 + px_l;
      const bool mine = x0 + px_l < v.pw;
      const bool col_in = (unsigned)gx < (unsigned)v.W;
      if (row_in) {
        if (mine && col_in)
          lds_dma16(vhead0 + (ptrdiff_t)(v.start + gy * v.W + v.px0 + x0) * (ptrdiff_t)pix_bytes, voff, lds0 + dst);
        if (mine && !col_in) *reinterpret_cast<u32x4*>(smem + dst + lane * 16) = u32x4{0u, 0u, 0u, 0u};
      } else if (mine) {
        *reinterpret_cast<u32x4*>(smem + dst + lane * 16) = u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
}

// ---- gather --------------------------------------------------------------------------------------------------------
// DPP hazard: a VGPR written by a vector instruction may be read by a DPP instruction only two wait states later.  The
// compiler inserts them for its own DPP forms but cannot see inside quad_bcast_add's inline assembly, and the addresses
// may have been written by the instruction right before (preparation directly in front of the gather: measured wrong
// results without this).  One s_nop per gather, tied to the address registers so that nothing moves across it.
__device__ __forceinline__ void dpp_guard(unsigned& a) { asm volatile("s_nop 1" : "+v"(a)); }
__device__ __forceinline__ void dpp_guard(unsigned& a, unsigned& b) { asm volatile("s_nop 1" : "+v"(a), "+v"(b)); }

// ---- output --------------------------------------------------------------------------------------------------------
// a (query, head) pair's lane: its 8 channels, rounded to nearest even, in one 16-byte store.  kAbl & 32: no output stores
// (timing experiments; the comparison keeps the accumulators alive)
template <class T, int kAbl>
__device__ __forceinline__ void store_out(unsigned char* const& orow, const int& q, const int& M, const float (&a)[8]) {
  const u32x4 o = {T::pack2(a[0], a[1]), T::pack2(a[2], a[3]), T::pack2(a[4], a[5]), T::pack2(a[6], a[7])};
  if (!(kAbl & 32) || o[0] == 0x12345678u) *reinterpret_cast<u32x4*>(orow + (size_t)((unsigned)q * ((unsigned)M * kRow))) = o;
}

}  // namespace
