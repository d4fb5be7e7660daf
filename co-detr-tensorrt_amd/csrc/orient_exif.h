// The host-only reader of a JPEG file's EXIF orientation (include/codetr_orient.h, codetr_orient_exif): plain C++, no HIP,
// so that the same text is compiled into libcodetr_hip.so and into a stand-alone host program under the sanitizers
// (tests/cabi_c/orient_exif_host_check.cpp).  It reads untrusted bytes: every read is bounded by `bytes`, and inside the
// Exif segment by the TIFF block's own length.
#ifndef CODETR_ORIENT_EXIF_H_
#define CODETR_ORIENT_EXIF_H_

#include <stdint.h>
#include <string.h>

namespace orient {

// the TIFF block of an Exif payload: t[0, T) -> 1..8
inline int tiff_orientation(const unsigned char* t, int64_t T) {
  if (T < 8) return 1;
  bool le;
  if (memcmp(t, "II*\0", 4) == 0) {
    le = true;
  } else if (memcmp(t, "MM\0*", 4) == 0) {
    le = false;
  } else {
    return 1;
  }
  // (callers keep at + 2 / at + 4 <= T)
  auto u16 = [&](int64_t at) -> int64_t { return le ? t[at] | (t[at + 1] << 8) : (t[at] << 8) | t[at + 1]; };
  auto u32 = [&](int64_t at) -> int64_t { return le ? u16(at) | (u16(at + 2) << 16) : (u16(at) << 16) | u16(at + 2); };
  const int64_t d = u32(4);
  if (d > T - 2) return 1;
  const int64_t n = u16(d);
  for (int64_t k = 0; k < n; ++k) {
    const int64_t e = d + 2 + 12 * k;
    if (e > T - 12) return 1;
    if (u16(e) != 0x0112) continue;
    if (u16(e + 2) != 3 || u32(e + 4) != 1) return 1;
    const int64_t v = u16(e + 8);
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 1;
}

// the whole file: f[0, n) with n > 0 -> 1..8
inline int exif_orientation(const unsigned char* f, int64_t n) {
  if (n < 2 || f[0] != 0xFF || f[1] != 0xD8) return 1;
  int64_t p = 2;
  while (p <= n - 4) {
    if (f[p] != 0xFF) return 1;
    const int m = f[p + 1];
    if (m == 0xFF) {   // a fill byte
      p += 1;
      continue;
    }
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {   // stand-alone markers
      p += 2;
      continue;
    }
    if (m == 0xDA || m == 0xD9) return 1;
    const int64_t len = (f[p + 2] << 8) | f[p + 3];
    if (len < 2 || len > n - (p + 2)) return 1;
    if (m == 0xE1 && len - 2 >= 6 && memcmp(f + p + 4, "Exif\0\0", 6) == 0) return tiff_orientation(f + p + 10, len - 8);
    p += 2 + len;
  }
  return 1;
}

}  // namespace orient

#endif  // CODETR_ORIENT_EXIF_H_
