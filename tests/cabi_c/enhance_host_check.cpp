// Host memory check of the contrast-enhancement stage's host side (csrc/enhance_args.h): a stand-alone program for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ico-detr-tensorrt_amd/csrc ...
// The argument checks on a row table that is a heap block of exactly its length, the geometry of a 1080p frame, and the
// multiplier of the header's division over sampled numerators.  Prints `checks ok`, then `clean`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "enhance_args.h"

static const int R = CODETR_ENHANCE_ROW_INTS;
static const uintptr_t SRC = 1 << 20, DST = 1 << 24, WS = 1 << 26;

static int call(const int64_t* rows, int64_t N, uintptr_t src = SRC, uintptr_t dst = DST, uintptr_t ws = WS, int64_t ws_bytes = 1 << 20) {
  const size_t n = N > 0 ? N : 1;
  int64_t* r = static_cast<int64_t*>(malloc(sizeof(int64_t) * R * n));
  memcpy(r, rows, sizeof(int64_t) * R * n);
  enhance::ImageTable* tab = new enhance::ImageTable;
  enhance::Launch g;
  const int rc = enhance::check(src, 4096, N, r, dst, 4096, ws, ws_bytes, tab, &g);
  if (rc == 0 && enhance::workspace_bytes(N, r) > ws_bytes) abort();
  delete tab;
  free(r);
  return rc;
}

int main() {
  // H, W, src offset, src pitch, dst offset, dst pitch, gy, gx, C: tiles of 2 x 3, one slice each
  const int64_t good[R] = {4, 5, 1, 17, 2, 16, 2, 2, 3};
  int64_t many[R * 33];
  for (int n = 0; n < 33; ++n) {
    memcpy(many + R * n, good, sizeof good);
    many[R * n + 4] = 2 + 63 * n;   // images back to back: 3 * 16 + 15 = 63 bytes each
  }
  if (call(good, 1) != 0 || call(many, 32) != 0 || call(many, 33) != CODETR_E_TOO_LARGE) return 2;
  if (enhance::workspace_bytes(32, many) != 32 * 4 * 1024 || enhance::workspace_bytes(33, many) != CODETR_E_TOO_LARGE) return 2;
  many[R + 4] -= 1;                 // the first two images share a byte
  if (call(many, 2) != CODETR_E_BADARG) return 2;
  const int big = CODETR_FRAME_MAX_SIDE + 1;
  const struct { int at; int64_t v; int want; } edits[] = {   // `good` with one value changed
      {0, 0, CODETR_E_BADARG}, {1, -2, CODETR_E_BADARG}, {0, big, CODETR_E_TOO_LARGE}, {1, big, CODETR_E_TOO_LARGE},
      {2, -1, CODETR_E_BADARG}, {3, 14, CODETR_E_BADARG}, {2, 4096 - 65, CODETR_E_BADARG},   // 3 * 17 + 15 = 66 bytes of rows
      {4, -1, CODETR_E_BADARG}, {5, 14, CODETR_E_BADARG}, {4, 4096 - 62, CODETR_E_BADARG}, {6, 0, CODETR_E_BADARG},
      {6, 5, CODETR_E_BADARG}, {7, 6, CODETR_E_BADARG}, {7, 33, CODETR_E_BADARG}, {8, 0, CODETR_E_BADARG}, {8, 7, CODETR_E_BADARG}};
  for (const auto& e : edits) {
    int64_t row[R];
    memcpy(row, good, sizeof row);
    row[e.at] = e.v;
    if (call(row, 1) != e.want) return 3;
  }
  int64_t edge[R];
  memcpy(edge, good, sizeof edge);
  edge[2] = 4096 - 66, edge[4] = 4096 - 63, edge[8] = 6;   // the last read and the last written byte are the buffers' last; C = T
  if (call(edge, 1) != 0) return 3;
  // in place: the same buffer, sizes, offsets and pitches -- and nothing else that overlaps
  int64_t same[R];
  memcpy(same, good, sizeof same);
  same[4] = same[2], same[5] = same[3];
  if (call(same, 1, SRC, SRC) != 0 || call(good, 1, SRC, SRC) != CODETR_E_BADARG || call(same, 1, SRC, SRC + 16) != CODETR_E_BADARG) return 4;
  if (call(good, 0) != CODETR_E_BADARG || call(good, 1, 0) != CODETR_E_BADARG || call(good, 1, SRC, 0) != CODETR_E_BADARG ||
      call(good, 1, SRC, DST, 0) != CODETR_E_BADARG || call(good, 1, SRC, DST, WS + 2) != CODETR_E_BADARG ||
      call(good, 1, SRC, DST, WS, 4095) != CODETR_E_BADARG || call(good, 1, SRC, DST, WS, 4096) != 0 ||
      call(good, 1, SRC, DST, DST + 4092, 4096) != CODETR_E_BADARG) return 5;
  // geometry: 1080p at 8 x 8 is tiles of 135 x 240 in 4 slices of 34 rows; at 1 x 1 the slice count is capped
  const int64_t hd[R] = {1080, 1920, 0, 5760, 0, 5760, 8, 8, 253}, one[R] = {1080, 1920, 0, 5760, 0, 5760, 1, 1, 1};
  const int64_t wide[R] = {32767, 32767, 0, 98301, 0, 98301, 1, 1, 1}, most[R] = {2048, 2048, 0, 6144, 0, 6144, 1, 1, 1};
  enhance::Image im;
  if (enhance::geometry(hd, &im) != 0 || im.th != 135 || im.tw != 240 || im.sr != 34 || im.S != 4 || im.br != 34 || im.bands != 4) return 6;
  if (enhance::geometry(one, &im) != 0 || im.S != 32 || im.sr != 34 || im.br != 4 || im.bands != 270) return 6;
  if (enhance::geometry(wide, &im) != CODETR_E_BADARG || enhance::geometry(most, &im) != 0 || im.T != CODETR_ENHANCE_MAX_TILE) return 6;
  // the header's division: q0 = (n M) >> 32 is floor(n / d) or one less, for the smallest, an odd and the largest T
  const uint64_t tiles[] = {1, 6, 32399, CODETR_ENHANCE_MAX_TILE};
  for (uint64_t T : tiles) {
    const uint64_t d = 4 * T, M = (uint64_t(1) << 32) / d, top = 1022 * T;
    for (uint64_t k = 0; k <= 4096; ++k) {
      const uint64_t n = k < 2048 ? top - (k < top ? k : top) : (top * (k - 2048)) / 2048, q0 = (n * M) >> 32;
      if (n >> 32 || (q0 + (n - q0 * d >= d ? 1 : 0)) != n / d) return 7;
    }
  }
  printf("checks ok\nclean\n");
  return 0;
}
