// Host check of csrc/msda_window_geom.h (tests/test_msda_window_cpu.py builds and runs it, under -fsanitize=address,undefined
// where the runtimes exist): the item a lane of the windowed MSDA kernels computes (region_item) against the host forms the
// planning uses (q_bound, ext_lo, ext_hi), and the property the kernels' window test relies on.  On the host idiv is exact
// division, so this pins the formulas, not the device's reciprocal.
//   usage: msda_window_host_check [R cap, default 64]      prints "<cases> clean" and returns 0, or the first failure and 1
#include <cstdio>
#include <cstdlib>

#include "msda_window_geom.h"

using namespace msda_win;

static long long g_cases = 0;

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      std::printf("FAILED %s: ", #cond);      \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      return false;                           \
    }                                         \
  } while (0)

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// item j of one axis: the axis's (r, n, R) go to the x arguments for j = 0, 1, 4, 5 and to the y arguments for 2, 3, 6, 7;
// the other axis gets values that must not matter
static int item(int j, int r, int n, int R, int off) {
  const auto offset = [&](bool) { return off; };
  return (j & 2) ? region_item(j, 1, r, 7, n, 3, R, offset) : region_item(j, r, 1, n, 7, R, 3, offset);
}
static int dividend(int j, int r, int n, int R, int off) { return region_dividend(j, region_num(j, r, n, R, off), R); }

static bool check_axis(int n, int R) {
  CHECK(q_bound(0, n, R) == 0 && q_bound(R, n, R) == n, "n %d R %d", n, R);
  for (int r = 0; r < R; ++r) {
    const int q0 = q_bound(r, n, R), q1 = q_bound(r + 1, n, R);
    CHECK(q0 <= q1, "q_bound not monotone: n %d R %d r %d", n, R, r);   // with the ends: every pixel in exactly one region
    for (int ax = 0; ax < 4; ax += 2) {
      CHECK(item(4 + ax, r, n, R, 0) == q0 && item(5 + ax, r, n, R, 0) == q1, "query bounds: n %d R %d r %d axis %d", n, R, r, ax);
      CHECK(dividend(4 + ax, r, n, R, 0) <= region_dividend_bound(n, R, 0) && dividend(5 + ax, r, n, R, 0) <= region_dividend_bound(n, R, 0),
            "query dividend: n %d R %d r %d", n, R, r);
    }
    for (int lo = -12; lo <= 12; ++lo) {
      const int first = ext_lo(r, n, R, lo);
      CHECK(item(0, r, n, R, lo) == first && item(2, r, n, R, lo) == first, "ext_lo: n %d R %d r %d lo %d", n, R, r, lo);
      for (int hi = lo; hi <= 12; ++hi) {
        const int last = ext_hi(r, n, R, hi, first);
        const int wmax = abs(lo) > abs(hi) ? abs(lo) : abs(hi);
        const long long bound = region_dividend_bound(n, R, wmax);
        for (int ax = 0; ax < 4; ax += 2) {
          const int raw = item(1 + ax, r, n, R, hi);
          CHECK((raw < first + 1 ? first + 1 : raw) == last, "ext_hi: n %d R %d r %d lo %d hi %d axis %d", n, R, r, lo, hi, ax);
          const int d0 = dividend(ax, r, n, R, lo), d1 = dividend(1 + ax, r, n, R, hi);
          CHECK(d0 <= bound && d1 <= bound, "dividend above its bound: n %d R %d r %d lo %d hi %d: %d %d > %lld", n, R, r, lo, hi, d0, d1, bound);
        }
        CHECK(-1 <= first && first < last && last <= n, "window: n %d R %d r %d lo %d hi %d: [%d, %d]", n, R, r, lo, hi, first, last);
        // what in_window relies on: a sample of a query pixel x of the region at an offset in [d, d + 1), d in [lo, hi], has
        // its corners x + d and x + d + 1 -- clamped to the zero border, beyond which nothing is read -- inside the window
        for (int x = q0; x < q1; ++x)
          for (int d = lo; d <= hi; ++d) {
            const int c0 = clampi(x + d, -1, n), c1 = clampi(x + d + 1, -1, n);
            CHECK(first <= c0 && c0 <= last && first <= c1 && c1 <= last, "corner outside: n %d R %d r %d lo %d hi %d x %d d %d: [%d, %d]", n, R,
                  r, lo, hi, x, d, first, last);
          }
        ++g_cases;
      }
    }
  }
  return true;
}

int main(int argc, char** argv) {
  const int rcap = argc > 1 ? atoi(argv[1]) : 64;
  for (int l = 0; l < kLevels; ++l) {
    const int want = l == 0 ? 0 : l <= 2 ? 1 : 3;
    if (pass_first(l) != want) return std::printf("FAILED pass_first(%d)\n", l), 1;
  }
  // the op's plan admits sides <= 4096, 16-pixel regions of the largest level and margins <= 12
  if (region_dividend_bound(4096, 256, 12) >= (1 << 22)) return std::printf("FAILED the op's dividend bound\n"), 1;
  const int big[3] = {1000, 4095, 4096};
  for (int i = 1; i <= 96 + 3; ++i) {
    const int n = i <= 96 ? i : big[i - 97];
    for (int R = 1; R <= (n < rcap ? n : rcap); ++R)
      if (!check_axis(n, R)) return 1;
  }
  std::printf("%lld clean\n", g_cases);
  return 0;
}
