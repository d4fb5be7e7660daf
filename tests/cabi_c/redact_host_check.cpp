// The argument checks of codetr_redact_detections_* (co-detr-tensorrt_amd/csrc/redact_args.h) as a stand-alone host
// program, for a run under -fsanitize=address,undefined: heap-allocated image tables of exactly the size a call reads, so
// a check that reads past its N rows is reported.  Prints "clean" and returns 0 when every call answers as expected.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "redact_args.h"

namespace {

int failures = 0;

void expect(int64_t got, int64_t want, const char* what) {
  if (got != want) {
    printf("FAIL %s: got %lld, expected %lld\n", what, (long long)got, (long long)want);
    ++failures;
  }
}

struct Call {
  std::vector<int64_t> images;
  int64_t buf_bytes, N, Q, C;
  const void *buf, *boxes, *scores, *work;
  const int64_t* labels;
  const int* count;
  const unsigned char* select;
  int mode, shape, cell;
  float thr, expand;
  uint32_t fill;
  int64_t work_bytes;
  redact_args::Table tab;
  int64_t Hmax, Wmax;

  int run() {
    // the table in a heap block of exactly 3 N words (N as the images vector holds them)
    int64_t* rows = images.empty() ? nullptr : static_cast<int64_t*>(malloc(images.size() * sizeof(int64_t)));
    for (size_t i = 0; i < images.size(); ++i) rows[i] = images[i];
    const int rc = redact_args::check(buf, buf_bytes, N, rows, boxes, scores, labels, count, Q, select, C, mode, shape, cell,
                                      thr, expand, fill, work, work_bytes, &tab, &Hmax, &Wmax);
    free(rows);
    return rc;
  }
};

Call good() {
  alignas(16) static unsigned char bytes[16];
  static int64_t labels[4];
  static int count[4];
  Call c;
  c.images = {1, 70, 131, 1 + 70 * 131 * 3 + 3, 5, 7};
  c.buf_bytes = 1 + 70 * 131 * 3 + 3 + 5 * 7 * 3;
  c.N = 2, c.Q = 16, c.C = 0;
  c.buf = c.boxes = c.scores = bytes;
  c.work = nullptr;
  c.labels = labels, c.count = count, c.select = nullptr;
  c.mode = CODETR_REDACT_PIXELATE, c.shape = CODETR_REDACT_BOX, c.cell = 16;
  c.thr = 0.3f, c.expand = 0.1f, c.fill = 0, c.work_bytes = 0;
  return c;
}

}  // namespace

int main() {
  {
    Call c = good();
    expect(c.run(), 0, "good");
    expect(c.Hmax, 70, "Hmax");
    expect(c.Wmax, 131, "Wmax");
    expect(c.tab.img[1].offset, 1 + 70 * 131 * 3 + 3, "offset of image 1");
    expect(c.tab.img[1].work, 5 * 9, "work offset of image 1");
    expect(c.tab.img[1].H, 5, "H of image 1");
  }
  for (int cell = 0; cell <= 130; ++cell) {
    Call c = good();
    c.cell = cell;
    const bool ok = cell == 4 || cell == 8 || cell == 16 || cell == 32 || cell == 64;
    expect(c.run(), ok ? 0 : CODETR_E_BADARG, "cell");
    const int64_t cells = redact_args::count_cells(2, c.images.data(), cell, nullptr);
    if (ok) expect(cells, ((70 + cell - 1) / cell) * ((131 + cell - 1) / cell) + ((5 + cell - 1) / cell) * ((7 + cell - 1) / cell), "cells");
    else expect(cells, CODETR_E_BADARG, "cells of a bad cell");
  }
#define CASE(WHAT, CODE, ...)   \
  {                             \
    Call c = good();            \
    __VA_ARGS__;                \
    expect(c.run(), CODE, WHAT); \
  }
  CASE("null buf", CODETR_E_BADARG, c.buf = nullptr)
  CASE("null images", CODETR_E_BADARG, c.images.clear())
  CASE("null boxes", CODETR_E_BADARG, c.boxes = nullptr)
  CASE("null scores", CODETR_E_BADARG, c.scores = nullptr)
  CASE("null labels", CODETR_E_BADARG, c.labels = nullptr)
  CASE("null count", CODETR_E_BADARG, c.count = nullptr)
  CASE("N = 0", CODETR_E_BADARG, c.N = 0)
  CASE("N < 0", CODETR_E_BADARG, c.N = -1)
  CASE("Q = 0", CODETR_E_BADARG, c.Q = 0)
  CASE("no bytes", CODETR_E_BADARG, c.buf_bytes = 0)
  CASE("a table without classes", CODETR_E_BADARG, c.select = static_cast<const unsigned char*>(c.buf))
  CASE("mode 3", CODETR_E_BADARG, c.mode = 3)
  CASE("mode -1", CODETR_E_BADARG, c.mode = -1)
  CASE("shape 2", CODETR_E_BADARG, c.shape = 2)
  CASE("NaN threshold", CODETR_E_BADARG, c.thr = 0.f / 0.f)
  CASE("expand < 0", CODETR_E_BADARG, c.expand = -0.25f)
  CASE("expand > 1", CODETR_E_BADARG, c.expand = 1.25f)
  CASE("NaN expand", CODETR_E_BADARG, c.expand = 0.f / 0.f)
  CASE("fill above 24 bits", CODETR_E_BADARG, c.fill = 0x1000000u)
  CASE("a row outside the buffer", CODETR_E_BADARG, c.buf_bytes -= 1)
  CASE("a negative offset", CODETR_E_BADARG, c.images[0] = -1)
  CASE("an offset behind the buffer", CODETR_E_BADARG, c.images[3] = c.buf_bytes + 1)
  CASE("overlapping images", CODETR_E_BADARG, c.images[3] = 100)
  CASE("H = 0", CODETR_E_BADARG, c.images[1] = 0)
  CASE("W < 0", CODETR_E_BADARG, c.images[5] = -7)
  CASE("blur without a workspace", CODETR_E_BADARG, c.mode = CODETR_REDACT_BLUR)
  CASE("blur with a small workspace", CODETR_E_BADARG, c.mode = CODETR_REDACT_BLUR; c.work = c.buf; c.work_bytes = 4 * 46 - 1)
  CASE("blur with a misaligned workspace", CODETR_E_BADARG, c.mode = CODETR_REDACT_BLUR;
       c.work = static_cast<const unsigned char*>(c.buf) + 2; c.work_bytes = 4096)
  CASE("blur", 0, c.mode = CODETR_REDACT_BLUR; c.work = c.buf; c.work_bytes = 4 * 46)
  CASE("a table", 0, c.select = static_cast<const unsigned char*>(c.buf); c.C = 4)
  CASE("N = 33", CODETR_E_TOO_LARGE, c.N = 33)
  CASE("Q = 4097", CODETR_E_TOO_LARGE, c.Q = 4097)
  CASE("C = 65537", CODETR_E_TOO_LARGE, c.select = static_cast<const unsigned char*>(c.buf); c.C = 65537)
  CASE("a side above the limit", CODETR_E_TOO_LARGE, c.images[1] = CODETR_DRAW_MAX_SIDE + 1; c.buf_bytes = (int64_t)1 << 40)
  CASE("one image", 0, c.N = 1; c.images.resize(3))
  {  // 32 images of the largest side: the sums stay inside int64 and the table is filled to its end
    Call c = good();
    c.N = CODETR_PREPROCESS_BATCH_MAX;
    c.images.clear();
    const int64_t side = CODETR_DRAW_MAX_SIDE, bytes = side * side * 3;
    for (int64_t n = 0; n < c.N; ++n) c.images.insert(c.images.end(), {n * bytes, side, side});
    c.buf_bytes = c.N * bytes;
    c.cell = 4;
    expect(c.run(), 0, "32 largest images");
    expect(c.tab.img[31].work, 31 * (side / 4) * (side / 4), "work offset of image 31");
  }
  if (failures) return 1;
  printf("clean\n");
  return 0;
}
