// Host memory check of the lens-undistortion stage's host side (csrc/undistort_args.h): a stand-alone program for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ico-detr-tensorrt_amd/csrc ...
// The argument checks on row and parameter tables that are heap blocks of exactly their length.  Prints `checks ok`, then
// `clean`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "undistort_args.h"

static const int R = CODETR_UNDISTORT_ROW_INTS, P = CODETR_UNDISTORT_PARAM_FLOATS;

static int call(const int64_t* rows, const float* params, int64_t N, uintptr_t src = 1 << 20, uintptr_t dst = 1 << 24) {
  const size_t n = N > 0 ? N : 1;
  int64_t* r = static_cast<int64_t*>(malloc(sizeof(int64_t) * R * n));
  float* p = static_cast<float*>(malloc(sizeof(float) * P * n));
  memcpy(r, rows, sizeof(int64_t) * R * n), memcpy(p, params, sizeof(float) * P * n);
  undistort::ImageTable* tab = new undistort::ImageTable;
  int64_t Hmax = 0, Wmax = 0;
  const int rc = undistort::check(src, 4096, N, r, p, dst, 4096, tab, &Hmax, &Wmax);
  if (rc == 0 && N == 1 && (Hmax != rows[5] || Wmax != rows[6] || tab->f[0].fill != 0x563412u)) abort();
  delete tab;
  free(p), free(r);
  return rc;
}

int main() {
  // model, H, W, src offset, pitch, H', W', dst offset, fill
  const int64_t good[R] = {CODETR_UNDISTORT_FISHEYE, 4, 5, 1, 17, 3, 7, 2, 0x123456};
  const float cam[P] = {300.f, 310.f, 2.5f, 2.f, 150.f, 150.f, 3.f, 1.f, -0.01f, 0.002f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int64_t many[R * 33];
  float cams[P * 33];
  for (int n = 0; n < 33; ++n) {
    memcpy(many + R * n, good, sizeof good), memcpy(cams + P * n, cam, sizeof cam);
    many[R * n + 7] = 2 + 63 * n;   // images back to back
  }
  if (call(good, cam, 1) != 0 || call(many, cams, 32) != 0 || call(many, cams, 33) != CODETR_E_TOO_LARGE) return 2;
  many[R + 7] -= 1;                 // the first two images share a byte
  if (call(many, cams, 2) != CODETR_E_BADARG) return 2;
  const int big = CODETR_FRAME_MAX_SIDE + 1;
  const struct { int at; int64_t v; int want; } edits[] = {   // `good` with one value changed
      {0, 2, CODETR_E_BADARG}, {0, -1, CODETR_E_BADARG}, {1, 0, CODETR_E_BADARG}, {2, 0, CODETR_E_BADARG}, {5, 0, CODETR_E_BADARG},
      {6, -3, CODETR_E_BADARG}, {1, big, CODETR_E_TOO_LARGE}, {5, big, CODETR_E_TOO_LARGE}, {6, big, CODETR_E_TOO_LARGE},
      {3, -1, CODETR_E_BADARG}, {4, 14, CODETR_E_BADARG}, {3, 4096 - 65, CODETR_E_BADARG},   // 3 * 17 + 15 = 66 bytes of rows
      {7, -1, CODETR_E_BADARG}, {7, 4096 - 62, CODETR_E_BADARG}, {8, -1, CODETR_E_BADARG}, {8, 0x1000000, CODETR_E_BADARG}};
  for (const auto& e : edits) {
    int64_t row[R];
    memcpy(row, good, sizeof row);
    row[e.at] = e.v;
    if (call(row, cam, 1) != e.want) return 3;
  }
  int64_t edge[R];
  memcpy(edge, good, sizeof edge);
  edge[3] = 4096 - 66, edge[7] = 4096 - 63;   // the last stored byte and the last written byte are the buffers' last
  if (call(edge, cam, 1) != 0) return 3;
  const struct { int at; float v; } bad[] = {{0, 0.f}, {1, -1.f}, {4, NAN}, {5, INFINITY}, {0, 16385.f}, {5, 16384.5f}, {2, 32769.f},
                                             {7, -40000.f}, {8, NAN}, {15, INFINITY}, {11, -INFINITY}};
  for (const auto& e : bad) {
    float p[P];
    memcpy(p, cam, sizeof p);
    p[e.at] = e.v;
    if (call(good, p, 1) != CODETR_E_BADARG) return 4;
  }
  float lim[P];
  memcpy(lim, cam, sizeof lim);
  lim[0] = 16384.f, lim[2] = -32768.f, lim[7] = 32768.f, lim[15] = 3e38f;   // the ends of the admitted ranges
  if (call(good, lim, 1) != 0) return 4;
  if (call(good, cam, 0) != CODETR_E_BADARG || call(good, cam, 1, 0) != CODETR_E_BADARG || call(good, cam, 1, 1 << 20, 0) != CODETR_E_BADARG ||
      call(good, cam, 1, 1 << 20, (1 << 20) + 4095) != CODETR_E_BADARG || call(good, cam, 1, 1 << 20, (1 << 20) + 4096) != 0) return 5;
  printf("checks ok\nclean\n");
  return 0;
}
