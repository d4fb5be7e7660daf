// Host memory check of the raw Bayer stage's host side (csrc/raw_args.h): a stand-alone program for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ico-detr-tensorrt_amd/csrc ...
// The fold rule against a walk of the reflection on every short axis, the multipliers at the edge settings, and the
// argument checks on row tables that are heap blocks of exactly their length.  Prints one line per part, then `clean`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "raw_args.h"

static int fold_by_walking(int i, int n) {  // the reflection, one step at a time
  int at = 0, step = 1;
  for (int k = 0; n > 1 && k < (i < 0 ? -i : i); ++k) {
    if (at + step < 0 || at + step >= n) step = -step;
    at += step;
  }
  return at;
}

static int call(const int64_t* rows, int64_t N, const int64_t* settings, uintptr_t src = 1 << 20, uintptr_t lut = 1 << 16,
                uintptr_t dst = 1 << 24) {
  const size_t bytes = sizeof(int64_t) * CODETR_RAW_ROW_INTS * (N > 0 ? N : 1);
  int64_t* block = static_cast<int64_t*>(malloc(bytes));
  memcpy(block, rows, bytes);
  raw::Checked* out = new raw::Checked;
  const int rc = raw::check(src, 4096, N, block, settings, lut, dst, 4096, out);
  delete out;
  free(block);
  return rc;
}

int main() {
  for (int n = 1; n <= 9; ++n)
    for (int i = -40; i <= 40; ++i) {
      const int f = raw::fold(i, n);
      if (f != fold_by_walking(i, n) || (n > 1 && ((f ^ i) & 1))) return 2;  // reflection keeps the parity
    }
  if (raw::fold(-2, 16384) != 2 || raw::fold(16385, 16384) != 16381) return 2;
  printf("fold ok\n");

  int64_t m[3];
  const double one[3] = {1.0, 1.0, 1.0}, big[3] = {1.0, 65536.0, 1.0}, nan[3] = {1.0, NAN, 1.0}, neg[3] = {-0.5, 1.0, 1.0};
  const double edge[3] = {0.0, 65535.0 / 65536.0, 1.0};
  if (!raw::multipliers(0, 255, one, m) || m[0] != 257ll * 65536 || !raw::multipliers(0, 65535, one, m) || m[1] != 65536) return 3;
  if (!raw::multipliers(65534, 65535, edge, m) || m[0] != 0 || m[1] != 4294836225ll || m[2] != 4294901760ll) return 3;
  if (raw::multipliers(65534, 65535, big, m) || raw::multipliers(0, 65535, big, m)) return 3;   // 2^32 and above
  if (raw::multipliers(5, 5, one, m) || raw::multipliers(9, 5, one, m) || raw::multipliers(-1, 5, one, m) ||
      raw::multipliers(0, 65536, one, m) || raw::multipliers(0, 255, nan, m) || raw::multipliers(0, 255, neg, m)) return 3;
  printf("multipliers ok\n");

  const int64_t s8[6] = {CODETR_RAW_MALVAR, 0, 255, 1, 2, 4294967295ll}, s12[6] = {CODETR_RAW_BILINEAR, 64, 4095, 1, 1, 1};
  const int64_t good8[7] = {CODETR_RAW_GBRG, 8, 4, 5, 1, 7, 3}, good12[7] = {CODETR_RAW_RGGB, 12, 4, 5, 2, 12, 0};
  int64_t many[7 * 33];
  for (int n = 0; n < 33; ++n) memcpy(many + 7 * n, good8, sizeof good8), many[7 * n + 6] = 3 + 60 * n;   // images back to back
  if (call(good8, 1, s8) != 0 || call(good12, 1, s12) != 0 || call(many, 32, s8) != 0 || call(many, 33, s8) != CODETR_E_TOO_LARGE) return 4;
  many[13] -= 1;                                                         // the first two images share a byte
  if (call(many, 2, s8) != CODETR_E_BADARG) return 4;
  memcpy(many + 7, good12, sizeof good12), many[13] = 100;               // two containers in one call
  if (call(many, 2, s8) != CODETR_E_BADARG) return 4;
  const struct { int at; int64_t v; int want; } edits[] = {   // good12 with one value changed
      {0, 4, CODETR_E_BADARG}, {0, -1, CODETR_E_BADARG}, {1, 7, CODETR_E_BADARG}, {1, 17, CODETR_E_BADARG},
      {2, 0, CODETR_E_BADARG}, {3, 0, CODETR_E_BADARG}, {2, CODETR_FRAME_MAX_SIDE + 1, CODETR_E_TOO_LARGE},
      {4, -1, CODETR_E_BADARG}, {4, 3, CODETR_E_BADARG}, {5, 8, CODETR_E_BADARG}, {5, 13, CODETR_E_BADARG},   // odd offset, pitch
      {4, 4096 - 44, CODETR_E_BADARG}, {6, 4096 - 59, CODETR_E_BADARG}, {6, -1, CODETR_E_BADARG}};            // one byte outside
  for (const auto& e : edits) {
    int64_t row[7];
    memcpy(row, good12, sizeof row);
    row[e.at] = e.v;
    if (call(row, 1, s12) != e.want) return 5;
  }
  const int64_t bad_settings[][6] = {{2, 0, 255, 1, 1, 1}, {0, -1, 255, 1, 1, 1}, {0, 255, 255, 1, 1, 1}, {0, 0, 256, 1, 1, 1},
                                     {0, 0, 255, -1, 1, 1}, {0, 0, 255, 1, 1, 4294967296ll}};
  for (const auto& s : bad_settings)
    if (call(good8, 1, s) != CODETR_E_BADARG) return 6;
  if (call(good8, 0, s8) != CODETR_E_BADARG || call(good8, 1, s8, 0) != CODETR_E_BADARG ||
      call(good8, 1, s8, 1 << 20, (1 << 16) + 8) != CODETR_E_BADARG || call(good12, 1, s12, (1 << 20) + 1) != CODETR_E_BADARG ||
      call(good8, 1, s8, 1 << 20, 1 << 16, (1 << 20) + 4095) != CODETR_E_BADARG) return 7;
  printf("checks ok\nclean\n");
  return 0;
}
