// The host-only header parser of include/codetr_jpeg_dec.h (codetr_jpegdec_parse): plain C++, no HIP, so that the same
// text is compiled into libcodetr_hip.so and into the host memory check (tests/cabi_c/jpeg_dec_host_check.cpp).  It reads
// untrusted bytes: every read is bounded by `bytes`, every table index by its table.
#ifndef CODETR_JPEG_DEC_PARSE_H_
#define CODETR_JPEG_DEC_PARSE_H_

#include <stdint.h>
#include <string.h>

#include "codetr_jpeg_dec.h"

namespace jpegdec {

static const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

enum { kQuantBytes = 256, kHuffBytes = 272 };   // the layout of CODETR_JPEGDEC_TABLE_BYTES: 4 x 64, then 8 x (16 + 256)

inline int parse(const unsigned char* f, int64_t n, int32_t* info, unsigned char* tables) {
  if (!f || !info || !tables || n < 4) return CODETR_E_BADARG;
  memset(info, 0, sizeof(int32_t) * CODETR_JPEGDEC_INFO_INTS);
  memset(tables, 0, CODETR_JPEGDEC_TABLE_BYTES);
  if (n > CODETR_JPEGDEC_MAX_FILE_BYTES) return CODETR_E_TOO_LARGE;
  if (f[0] != 0xFF || f[1] != 0xD8) return CODETR_E_BADARG;
  unsigned reasons = 0;   // bit r: CODETR_JPEGDEC_R_<r> holds
  bool have_q[4] = {false, false, false, false}, have_h[8] = {};
  bool have_sof = false, too_large = false;
  int comp_id[4] = {0, 0, 0, 0}, ncomp = 0;
  int64_t p = 2;
  for (;;) {
    if (p + 2 > n) return CODETR_E_BADARG;
    if (f[p] != 0xFF) return CODETR_E_BADARG;
    const int m = f[p + 1];
    if (m == 0xFF) {   // a fill byte
      p += 1;
      continue;
    }
    p += 2;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // stand-alone markers
    if (m == 0x00 || m == 0xD8 || m == 0xD9) return CODETR_E_BADARG;
    if (p + 2 > n) return CODETR_E_BADARG;
    const int64_t len = (f[p] << 8) | f[p + 1];
    if (len < 2 || p + len > n) return CODETR_E_BADARG;
    const unsigned char* s = f + p + 2;
    const int64_t sl = len - 2;
    if (m == 0xDB) {   // DQT
      int64_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (tq > 3 || pq > 1) return CODETR_E_BADARG;
        const int64_t sz = pq ? 128 : 64;
        if (q + 1 + sz > sl) return CODETR_E_BADARG;
        if (pq) {
          reasons |= 1u << CODETR_JPEGDEC_R_QUANT16;
        } else {
          for (int k = 0; k < 64; ++k) tables[tq * 64 + kZigzag[k]] = s[q + 1 + k];
          have_q[tq] = true;
        }
        q += 1 + sz;
      }
    } else if (m == 0xC4) {   // DHT
      int64_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return CODETR_E_BADARG;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return CODETR_E_BADARG;
        int total = 0, code = 0;
        for (int l = 0; l < 16; ++l) {
          const int c = s[q + 1 + l];
          total += c;
          code += c;
          if (code > (1 << (l + 1))) return CODETR_E_BADARG;   // more codes of this length than the prefix leaves
          code <<= 1;
        }
        if (total > 256 || q + 17 + total > sl) return CODETR_E_BADARG;
        unsigned char* t = tables + kQuantBytes + (tc * 4 + th) * kHuffBytes;
        memset(t, 0, kHuffBytes);
        memcpy(t, s + q + 1, 16);
        memcpy(t + 16, s + q + 17, (size_t)total);
        have_h[tc * 4 + th] = true;
        q += 17 + total;
      }
    } else if (m == 0xDD) {   // DRI
      if (sl != 2) return CODETR_E_BADARG;
      info[3] = (s[0] << 8) | s[1];
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {   // SOFn
      if (have_sof) return CODETR_E_BADARG;
      if (sl < 6) return CODETR_E_BADARG;
      const int prec = s[0], H = (s[1] << 8) | s[2], W = (s[3] << 8) | s[4];
      ncomp = s[5];
      if (sl != 6 + 3 * (int64_t)ncomp || ncomp < 1) return CODETR_E_BADARG;
      if (H == 0 || W == 0) return CODETR_E_BADARG;
      have_sof = true;
      info[0] = H;
      info[1] = W;
      info[2] = ncomp;
      if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) too_large = true;
      if (m == 0xC2) reasons |= 1u << CODETR_JPEGDEC_R_PROGRESSIVE;
      else if (m == 0xC1) reasons |= 1u << CODETR_JPEGDEC_R_EXTENDED;
      else if (m == 0xC3) reasons |= 1u << CODETR_JPEGDEC_R_LOSSLESS;
      else if (m >= 0xC5 && m <= 0xC7) reasons |= 1u << CODETR_JPEGDEC_R_HIERARCHICAL;
      else if (m >= 0xC9) reasons |= 1u << CODETR_JPEGDEC_R_ARITHMETIC;
      if (m == 0xC0 && prec != 8) reasons |= 1u << CODETR_JPEGDEC_R_PRECISION;
      if (ncomp != 1 && ncomp != 3) {
        reasons |= 1u << CODETR_JPEGDEC_R_COMPONENTS;
      } else {
        for (int c = 0; c < ncomp; ++c) {
          comp_id[c] = s[6 + 3 * c];
          const int h = s[7 + 3 * c] >> 4, v = s[7 + 3 * c] & 15, tq = s[8 + 3 * c];
          if (h < 1 || h > 4 || v < 1 || v > 4 || tq > 3) return CODETR_E_BADARG;
          info[9 + 5 * c] = h;
          info[10 + 5 * c] = v;
          info[11 + 5 * c] = tq;
        }
        if (ncomp == 1) {
          info[9] = info[10] = 1;
        } else {
          if (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') reasons |= 1u << CODETR_JPEGDEC_R_RGB_IDS;
          const bool chroma11 = info[14] == 1 && info[15] == 1 && info[19] == 1 && info[20] == 1;
          const int h = info[9], v = info[10];
          if (!chroma11 || !((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)))
            reasons |= 1u << CODETR_JPEGDEC_R_SAMPLING;
        }
      }
    } else if (m == 0xEE) {   // APP14: "Adobe", version, flags0, flags1, transform
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0 && s[11] != 1) reasons |= 1u << CODETR_JPEGDEC_R_ADOBE;
    } else if (m == 0xDA) {   // SOS
      if (!have_sof) return CODETR_E_BADARG;
      if (sl < 1) return CODETR_E_BADARG;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sl != 4 + 2 * (int64_t)ns) return CODETR_E_BADARG;
      const int64_t scan = p + len;
      int64_t eoi = -1;
      for (int64_t q = n - 2; q >= scan; --q)
        if (f[q] == 0xFF && f[q + 1] == 0xD9) {
          eoi = q;
          break;
        }
      if (eoi < 0) return CODETR_E_BADARG;
      info[4] = (int32_t)scan;
      info[5] = (int32_t)(eoi - scan);
      if (too_large) return CODETR_E_TOO_LARGE;
      if (ns != ncomp) reasons |= 1u << CODETR_JPEGDEC_R_MULTISCAN;
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) reasons |= 1u << CODETR_JPEGDEC_R_SCAN_PARAMS;
      if (!reasons) {
        for (int c = 0; c < ncomp; ++c) {
          const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
          if (s[1 + 2 * c] != comp_id[c] || td > 3 || ta > 3) return CODETR_E_BADARG;
          if (!have_h[td] || !have_h[4 + ta] || !have_q[info[11 + 5 * c]]) return CODETR_E_BADARG;
          info[12 + 5 * c] = td;
          info[13 + 5 * c] = ta;
        }
        const int hmax = info[9], vmax = info[10];   // (chroma is 1x1, so luma holds the maxima)
        info[7] = hmax;
        info[8] = vmax;
        info[24] = (info[1] + 8 * hmax - 1) / (8 * hmax);
        info[25] = (info[0] + 8 * vmax - 1) / (8 * vmax);
        info[26] = ncomp == 1 ? 1 : hmax * vmax + 2;
        const int64_t blocks = (int64_t)info[24] * info[25] * info[26];
        if (blocks > 0x7FFFFFFF / 64) return CODETR_E_TOO_LARGE;
        info[27] = (int32_t)blocks;
        return 0;
      }
      for (int r = 1; r < 32; ++r)
        if (reasons >> r & 1u) {
          info[6] = r;
          break;
        }
      return CODETR_E_UNSUPPORTED;
    }
    // (every other segment -- APPn, COM, DAC, DNL, ... -- is skipped by its length)
    p += len;
  }
}

}  // namespace jpegdec
#endif  // CODETR_JPEG_DEC_PARSE_H_
