// Region / window geometry of the windowed MSDA kernels (csrc/msda_encoder4.hip, csrc/msda_op4.hip), in one place: the
// reciprocal division, the pass structure, the host forms of a region's query rectangle and staged window along one axis,
// and the item a lane of the kernels computes for them.  Plain C++: the kernels' host planning (plan4, make_plan) and a
// host-only check (tests/cabi_c/msda_window_host_check.cpp, g++) include it as well as the device code.
#pragma once

#if defined(__HIPCC__)
#define MSDA_HD __host__ __device__ __forceinline__
#else
#define MSDA_HD inline
#endif

namespace msda_win {

constexpr int kLevels = 5;   // the pass structure below is that of a five-level pyramid

// floor(a / b) for 0 <= a < 2^22, 0 < b.  Device: one float reciprocal + an exact fix-up (a 32-bit integer division is ~40
// instructions, and the general kernel evaluates the op's plan in every workgroup of its skipped launch).
MSDA_HD int idiv(int a, int b) {
#ifdef __HIP_DEVICE_COMPILE__
  int q = (int)((float)a * __builtin_amdgcn_rcpf((float)b));
  const int r = a - q * b;
  q += r >= b ? 1 : 0;
  q -= r < 0 ? 1 : 0;
  return q;
#else
  return a / b;
#endif
}
MSDA_HD int cdiv(int a, int b) { return idiv(a + b - 1, b); }

// first level of the pass a level belongs to: passes {0}, {1, 2}, {3, 4} (a pass's windows share the LDS buffer)
MSDA_HD constexpr int pass_first(int l) { return l == 0 ? 0 : l <= 2 ? 1 : 3; }

// ---- region geometry along one axis (n pixels, R regions): pixel x belongs to region r iff (x + 0.5) / n in [r / R, (r + 1) / R)
MSDA_HD int q_bound(int r, int n, int R) { return (2 * r * n + R - 1) / (2 * R); }
// staged columns for offsets in [lo, hi], in EXTENDED coordinates (-1 and n are the zero border):
//   first = floor(r n / R - 1/2 + lo) clamped to [-1, n - 1]; last = ceil((r + 1) n / R - 1/2 + hi) clamped to [first + 1, n]
MSDA_HD int ext_lo(int r, int n, int R, int lo) {
  const int num = 2 * r * n - R + 2 * lo * R;
  const int v = num < 0 ? -1 : num / (2 * R);
  return v > n - 1 ? n - 1 : v;
}
MSDA_HD int ext_hi(int r, int n, int R, int hi, int first) {
  const int num = 2 * (r + 1) * n - R + 2 * hi * R;
  int v = num <= 0 ? 0 : (num + 2 * R - 1) / (2 * R);
  v = v > n ? n : v;
  return v < first + 1 ? first + 1 : v;
}

// ---- the same, as the kernels compute it: eight items per (level, region), one per lane (lane 8 l + j: item j of level l),
// each ONE division.  Items 0, 1, 4, 5 lie along x: (r, n, R) = (rx, W, RX); items 2, 3, 6, 7 along y: (ry, H, RY).
// offset(plus) gives the signed window offset of the item's side (pixels of the level; unused for j >= 4): the byte of the
// encoder kernel's (head, level) window, the op kernel's -margin / +margin.  It is a callable so that the kernels form
// the offset where they always did, after the item's axis and side: handed over as a value it moved in front of them and
// the kernels' listings changed.
//   item 0 / 2 == ext_lo(r, n, R, offset)                                        first staged column / row
//   item 1 / 3, raised to at least (item 0 / 2) + 1, == ext_hi(r, n, R, offset, item 0 / 2)    last staged column / row
//   item 4 / 6 == q_bound(r, n, R), item 5 / 7 == q_bound(r + 1, n, R)           the region's first query, the next region's
// (tests/test_msda_window_cpu.py holds the two forms together.)  region_num is the numerator before rounding,
// region_dividend what goes into idiv; region_dividend_bound bounds it over the regions, levels and offsets of a call.
MSDA_HD int region_num(int j, int r, int n, int R, int offset) {
  const bool isq = j >= 4, plus = (j & 1) != 0;
  const int rr = r + (plus ? 1 : 0);
  return 2 * rr * n + (isq ? R - 1 : 2 * offset * R - R);
}
MSDA_HD int region_dividend(int j, int num, int R) {
  const bool isq = j >= 4, plus = (j & 1) != 0;
  const int numd = (!isq && plus) ? num + 2 * R - 1 : num;
  return numd > 0 ? numd : 0;
}
template <class Offset>
MSDA_HD int region_item(int j, int rx, int ry, int W, int H, int RX, int RY, Offset&& offset) {
  const bool ay = (j & 2) != 0, isq = j >= 4, plus = (j & 1) != 0;
  const int n = ay ? H : W, R = ay ? RY : RX, r = ay ? ry : rx;
  const int num = region_num(j, r, n, R, offset(plus));
  const int q = idiv(region_dividend(j, num, R), 2 * R);
  return isq ? q : plus ? (num <= 0 ? 0 : (q > n ? n : q)) : (num < 0 ? -1 : (q > n - 1 ? n - 1 : q));
}
// every dividend of an axis with n pixels, R regions and offsets of magnitude <= wmax is at most this; the device idiv is
// exact below 2^22
MSDA_HD long long region_dividend_bound(int n, int R, int wmax) {
  return 2 * (long long)(R + 1) * n + (2 * (long long)wmax + 3) * R;
}

}  // namespace msda_win
