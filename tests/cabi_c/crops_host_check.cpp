// The argument checks and integer rules of co-detr-tensorrt_amd/csrc/crops_args.h as a stand-alone host program, for a run
// under -fsanitize=address,undefined: a heap image table of exactly the size a call reads, the tap arithmetic at the
// header's limits (signed overflow is reported).  Prints "clean" and returns 0 when every call answers as expected.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "crops_args.h"

static int failures = 0;
static void expect(int64_t got, int64_t want, const char* what) {
  if (got != want) printf("FAIL %s: got %lld, expected %lld\n", what, (long long)got, (long long)want), ++failures;
}

struct Call {
  std::vector<int64_t> images = {1, 70, 131, 1 + 70 * 131 * 3 + 3, 5, 7};
  int64_t bytes = 1 + 70 * 131 * 3 + 3 + 5 * 7 * 3, N = 2, Q = 16, C = 0, Wmax = 0;
  const void *ptr = &Wmax, *tensor = nullptr;
  const int* table = reinterpret_cast<const int*>(&Wmax);
  const unsigned char* select = nullptr;
  int w = 16, h = 8, M = 4, fit = CODETR_CROPS_STRETCH, type = CODETR_CROPS_TENSOR_NONE;
  float thr = 0.3f, expand = 0.f, mean[3] = {1, 2, 3}, stdv[3] = {4, 5, 6};
  uint32_t pad = 0x727272u;
  crops_args::Table tab;
  int run() {
    int64_t* rows = static_cast<int64_t*>(malloc(images.size() * sizeof(int64_t)));  // exactly 3 N words
    for (size_t i = 0; i < images.size(); ++i) rows[i] = images[i];
    const int rc = crops_args::check(ptr, bytes, N, rows, ptr, ptr, static_cast<const int64_t*>(ptr), table, Q, select, C, w, h,
                                     M, fit, thr, expand, pad, ptr, table, table, tensor, type, mean, stdv, &tab, &Wmax);
    free(rows);
    return rc;
  }
};

#define CASE(WHAT, CODE, ...)    \
  {                              \
    Call c;                      \
    __VA_ARGS__;                 \
    expect(c.run(), CODE, WHAT); \
  }

int main() {
  CASE("good", 0, (void)0)
  CASE("the largest output and a tensor", 0, c.w = c.h = 512; c.M = 256; c.type = CODETR_CROPS_TENSOR_BF16; c.tensor = c.ptr)
  CASE("w = 7", CODETR_E_BADARG, c.w = 7)
  CASE("expand > 1", CODETR_E_BADARG, c.expand = 1.25f)
  CASE("a misaligned table", CODETR_E_BADARG, c.table = reinterpret_cast<const int*>(static_cast<const char*>(c.ptr) + 2))
  CASE("a misaligned tensor", CODETR_E_BADARG, c.type = CODETR_CROPS_TENSOR_F16; c.tensor = static_cast<const char*>(c.ptr) + 1)
  CASE("a zero divisor", CODETR_E_BADARG, c.type = CODETR_CROPS_TENSOR_F32; c.tensor = c.ptr; c.stdv[1] = 0.f)
  CASE("a row outside the buffer", CODETR_E_BADARG, c.bytes -= 1)
  CASE("N = 33", CODETR_E_TOO_LARGE, c.N = 33)
  CASE("h = 513", CODETR_E_TOO_LARGE, c.h = 513)
  CASE("a side above the limit", CODETR_E_TOO_LARGE, c.images[1] = CODETR_DRAW_MAX_SIDE + 1; c.bytes = (int64_t)1 << 40)
  for (int n : {1, 8, 512})  // the tap rules at the limits: the largest region onto one sample, and one pixel onto 512
    for (int R : {1, 3, CODETR_DRAW_MAX_SIDE})
      for (int j : {0, n / 2, n - 1}) {
        int lo, hi;
        crops_args::tap_range(j, n, R, &lo, &hi);
        uint64_t sum = 0;
        for (int s = lo; s <= hi; ++s) sum += (uint64_t)crops_args::tap_weight(j, s, n, R);
        expect(lo > 0 ? crops_args::tap_weight(j, lo - 1, n, R) : 0, 0, "no weight below the range");
        expect(hi < R - 1 ? crops_args::tap_weight(j, hi + 1, n, R) : 0, 0, "no weight above the range");
        expect(sum > 0 && sum < ((uint64_t)1 << 30), 1, "0 < normaliser < 2^30");
      }
  int ox, oy, iw, ih;
  crops_args::inner_rect(CODETR_CROPS_PAD, CODETR_DRAW_MAX_SIDE, 1, 512, 512, &ox, &oy, &iw, &ih);
  expect(iw * 10000 + ih * 1000 + oy, 512 * 10000 + 1000 + 255, "pad: a flat region keeps one centred row");
  crops_args::inner_rect(CODETR_CROPS_PAD, 53, 37, 16, 8, &ox, &oy, &iw, &ih);
  expect(iw * 1000 + ih * 100 + ox * 10 + oy, 11 * 1000 + 8 * 100 + 2 * 10, "pad: 53 x 37 in 16 x 8");
  if (failures) return 1;
  printf("clean\n");
  return 0;
}
