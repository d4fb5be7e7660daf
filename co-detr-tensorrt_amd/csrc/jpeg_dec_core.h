// The decoder of include/codetr_jpeg_dec.h, written once for the kernels of jpeg_dec.hip and for the host: the bit
// reader, the symbol step over one chunk, the IDCT of one block and the upsampling + colour of one pixel.  Everything is
// __host__ __device__ and free of HIP calls, so tests/cabi_c/jpeg_dec_host_check.cpp compiles the very same text with a
// plain host compiler and runs it under the address sanitizer.  Every read of the scan is bounded by its length, every
// table index is masked to its table, every loop is counted.
#ifndef CODETR_JPEG_DEC_CORE_H_
#define CODETR_JPEG_DEC_CORE_H_

#include <stdint.h>

#include "codetr_jpeg_dec.h"

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

namespace jpegdec {

enum { kChunk = CODETR_JPEGDEC_CHUNK_BYTES, kRun = CODETR_JPEGDEC_RUN_CHUNKS, kDead = -1 };
// a lane's steps: every step consumes a bit of its chunk, jumps over a marker (2 bytes) or ends the decode
enum { kMaxSteps = 8 * kChunk + 40 };

struct Huff {              // canonical decoding tables (T.81 F.2.2.3) of DC tables 0..3 and AC tables 0..3
  int maxcode[8][16];      // the largest code of length l + 1, -1 when there is none
  int valoff[8][16];       // index into vals of a code c of that length: valoff + c
  unsigned char vals[8][256];
};

struct Scan {
  const unsigned char* data;   // the scan: stuffed, with its RSTm
  int len;
  int dri, bpm, nblocks;       // restart interval in MCUs, blocks per MCU, blocks of the image
  unsigned char comp[6];       // component of block i of the MCU
  unsigned char td[3], ta[3];  // the components' DC / AC tables
};

struct Lane {   // what a lane knows after decoding its chunk
  int pos, mk;  // exit state: pos = p * 8 + b or kDead; mk = blk * 64 + k
  int nblk;     // blocks completed
  int reset;    // 1 when the predictors were reset inside (then dc[] counts from the last reset)
  int dc[3];    // the predictors at the end, counted from the entry's (or from the last reset)
  int err;      // FINAL only: the first CODETR_JPEGDEC_S_* met before the image's last block was complete
};

JD_HD void huff_build(const unsigned char* bits_vals, int t, Huff* h) {   // bits_vals: BITS[16] HUFFVAL[256]
  int code = 0, k = 0;
  for (int l = 0; l < 16; ++l) {
    const int n = bits_vals[l];
    h->valoff[t][l] = k - code;
    h->maxcode[t][l] = n ? code + n - 1 : -1;
    k += n;
    code = (code + n) << 1;
  }
  for (int i = 0; i < 256; ++i) h->vals[t][i] = bits_vals[16 + i];
}

JD_HD int next_pos(const Scan& s, int p) {   // the byte behind data byte p
  return (s.data[p] == 0xFF && p + 1 < s.len && s.data[p + 1] == 0) ? p + 2 : p + 1;
}

JD_HD bool rst_at(const Scan& s, int q) { return q >= 0 && q + 1 < s.len && s.data[q] == 0xFF && (s.data[q + 1] & 0xF8) == 0xD0; }

// the next 32 bits at (p, b), zeros behind a stop; *avail of them are real; *stop: where the reader was stopped, or -1.
// Straight-line on purpose (five predicated byte steps, 32-bit words): no early exit for the compiler to restructure.
JD_HD uint32_t peek(const Scan& s, int p, int b, int* avail, int* stop) {
  uint32_t hi = 0, lo = 0;
  int cnt = 0, q = p, halted_at = -1;
  bool halted = false;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const bool inside = q >= 0 && q < s.len;
    const uint32_t v = inside ? (uint32_t)s.data[inside ? q : 0] : 0u;
    const bool ff = inside && v == 0xFFu;
    const bool stuffed = ff && q + 1 < s.len && s.data[(ff && q + 1 < s.len) ? q + 1 : 0] == 0;
    if (!halted && (!inside || (ff && !stuffed))) {
      halted = true;
      halted_at = q;
    }
    if (!halted) {
      if (i < 4) hi |= v << (24 - 8 * i);
      else lo = v;
      cnt += 1;
      q += stuffed ? 2 : 1;
    }
  }
  *stop = halted_at;
  const int a = cnt * 8 - b;
  *avail = a < 0 ? 0 : (a > 32 ? 32 : a);
  return b ? (hi << b) | (lo >> (8 - b)) : hi;
}

JD_HD int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

__attribute__((unused)) static const unsigned char kNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Decodes the symbols that start in [.., chunk_end) from the entry state (pos, mk); a dead entry state stands for the
// guess (chunk_begin, block 0, index 0).  FINAL: first_blk and pred_in are
// the image's block count and predictors at the entry; coefficients go to coef (nblocks x 64 int16, zero beforehand),
// natural[] is the zigzag -> natural map (in LDS on the device).
template <bool FINAL>
JD_HD void decode_chunk(const Scan& s, const Huff& h, const unsigned char* natural, int pos, int mk, int chunk_begin,
                        int chunk_end, int first_blk, const int* pred_in, short* coef, Lane* out) {
  Lane o;
  o.pos = pos;
  o.mk = mk;
  o.nblk = 0;
  o.reset = 0;
  o.err = 0;
  for (int c = 0; c < 3; ++c) o.dc[c] = FINAL ? pred_in[c] : 0;
  if (pos < 0) {   // the decode in front ended: this lane keeps its guess, so that the lanes behind can still settle
    pos = chunk_begin * 8;
    mk = 0;
  }
  int p = pos >> 3, b = pos & 7, blk = mk >> 6, k = mk & 63;
  if (blk >= s.bpm) blk = 0;   // (never from a state this code wrote)
  bool dead = false;
#define JD_ERR(code)                                                        \
  do {                                                                      \
    if (FINAL && !o.err && first_blk + o.nblk < s.nblocks) o.err = (code);  \
  } while (0)
  for (int step = 0; step < kMaxSteps && p < chunk_end; ++step) {
    int avail, stop;
    const uint32_t w = peek(s, p, b, &avail, &stop);
    const int comp = s.comp[blk] < 3 ? s.comp[blk] : 0;
    const int t = k == 0 ? (s.td[comp] & 3) : 4 + (s.ta[comp] & 3);
    const int top = (int)(w >> 16);
    int len = 0, sym = 0;
    for (int l = 1; l <= 16; ++l) {
      const int code = top >> (16 - l);
      if (code <= h.maxcode[t][l - 1]) {
        len = l;
        sym = h.vals[t][(h.valoff[t][l - 1] + code) & 255];
        break;
      }
    }
    bool stopped = false;
    int ssss = 0;
    if (!len) {
      if (avail >= 16) {
        JD_ERR(CODETR_JPEGDEC_S_BAD_CODE);
        dead = true;
        break;
      }
      stopped = true;
    } else if (len > avail) {
      stopped = true;
    } else if (k == 0 && sym > 15) {
      JD_ERR(CODETR_JPEGDEC_S_DC_CATEGORY);
      dead = true;
      break;
    } else {
      ssss = k == 0 ? sym : (sym & 15);
      if (len + ssss > avail) stopped = true;
    }
    if (stopped) {
      if (rst_at(s, stop)) {   // a marker inside a symbol: an error, and a true synchronisation point
        JD_ERR(CODETR_JPEGDEC_S_RST);
        p = stop + 2;
        b = 0;
        blk = 0;
        k = 0;
        o.reset = 1;
        o.dc[0] = o.dc[1] = o.dc[2] = 0;
        continue;
      }
      JD_ERR(CODETR_JPEGDEC_S_EXHAUSTED);
      dead = true;
      break;
    }
    int v = 0;
    if (ssss) {
      v = (int)((w << len) >> (32 - ssss));
      if (v < (1 << (ssss - 1))) v -= (1 << ssss) - 1;
    }
    const int g = first_blk + o.nblk;   // FINAL: the block this symbol belongs to
    bool done = false;
    if (k == 0) {
      o.dc[comp] = (int)((unsigned)o.dc[comp] + (unsigned)v);
      if (FINAL && g < s.nblocks) coef[(int64_t)g * 64] = (short)sat16(o.dc[comp]);
      k = 1;
    } else if (ssss == 0) {
      if ((sym >> 4) == 15) {
        k += 16;
        if (k > 63) {
          JD_ERR(CODETR_JPEGDEC_S_INDEX);
          dead = true;
          break;
        }
      } else {
        done = true;
      }
    } else {
      k += sym >> 4;
      if (k > 63) {
        JD_ERR(CODETR_JPEGDEC_S_INDEX);
        dead = true;
        break;
      }
      if (FINAL && g < s.nblocks) coef[(int64_t)g * 64 + natural[k]] = (short)v;
      k += 1;
      if (k == 64) done = true;
    }
    b += len + ssss;
    for (int i = 0; i < 4 && b >= 8; ++i) {
      p = next_pos(s, p);
      b -= 8;
    }
    if (done) {
      o.nblk += 1;
      k = 0;
      blk += 1;
      if (blk >= s.bpm) {
        blk = 0;
        const int q = b ? next_pos(s, p) : p;
        const bool rst = rst_at(s, q);
        if (FINAL) {
          const int gg = first_blk + o.nblk;   // blocks complete
          if (gg < s.nblocks) {
            const int M = gg / s.bpm;
            const bool expected = s.dri > 0 && M % s.dri == 0;
            if (rst && !expected) JD_ERR(CODETR_JPEGDEC_S_INTERVAL);
            else if (rst && (s.data[q + 1] & 7) != ((M / s.dri - 1) & 7)) JD_ERR(CODETR_JPEGDEC_S_RST);
            else if (!rst && expected) JD_ERR(CODETR_JPEGDEC_S_RST);
          }
        }
        if (rst) {
          p = q + 2;
          b = 0;
          o.reset = 1;
          o.dc[0] = o.dc[1] = o.dc[2] = 0;
        }
      }
    }
  }
#undef JD_ERR
  o.pos = dead ? (int)kDead : p * 8 + b;
  o.mk = dead ? 0 : blk * 64 + k;
  *out = o;
}

// ---- the pixel stage ---------------------------------------------------------------------------------------------------------
JD_HD void idct_1d(const int32_t* v, int stride, int32_t* out, int ostride, int shift) {
  typedef uint32_t u;
  const u v0 = (u)v[0], v1 = (u)v[stride], v2 = (u)v[2 * stride], v3 = (u)v[3 * stride], v4 = (u)v[4 * stride],
          v5 = (u)v[5 * stride], v6 = (u)v[6 * stride], v7 = (u)v[7 * stride];
  u z1 = (v2 + v6) * 4433u;
  const u t2 = z1 - v6 * 15137u, t3 = z1 + v2 * 6270u;
  const u t0 = (v0 + v4) << 13, t1 = (v0 - v4) << 13;
  const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  u a0 = v7, a1 = v5, a2 = v3, a3 = v1;
  z1 = a0 + a3;
  u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const u z5 = (z3 + z4) * 9633u;
  a0 *= 2446u;
  a1 *= 16819u;
  a2 *= 25172u;
  a3 *= 12299u;
  z1 *= (u)-7373;
  z2 *= (u)-20995;
  z3 = z3 * (u)-16069 + z5;
  z4 = z4 * (u)-3196 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  const u r = 1u << (shift - 1);
  const u x[8] = {t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3};
  for (int i = 0; i < 8; ++i) out[i * ostride] = (int32_t)(x[i] + r) >> shift;
}

JD_HD int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one 8x8 block: dequantise, both passes, level shift -> 64 samples, row-major with `pitch` bytes between rows
JD_HD void idct_block(const short* coef, const unsigned char* q, unsigned char* dst, int64_t pitch) {
  int32_t a[64], t[64];
  for (int i = 0; i < 64; ++i) a[i] = (int32_t)((uint32_t)(int32_t)coef[i] * (uint32_t)q[i]);
  for (int c = 0; c < 8; ++c) idct_1d(a + c, 8, t + c, 8, 11);
  for (int r = 0; r < 8; ++r) idct_1d(t + 8 * r, 1, a + 8 * r, 1, 18);
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) dst[r * pitch + c] = (unsigned char)clamp255(a[8 * r + c] + 128);
}

// the chroma sample of pixel (x, y): plane of `pitch` bytes per row with a real grid of dw x dh; hs, vs: 1 or 2
JD_HD int upsample(const unsigned char* pl, int64_t pitch, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return pl[(int64_t)(vs == 2 ? y >> 1 : y) * pitch + x];
  const int i = x >> 1;
  if (dw <= 2) return pl[(int64_t)(vs == 2 ? y >> 1 : y) * pitch + i];
  if (vs == 1) {
    const unsigned char* r = pl + (int64_t)y * pitch;
    if (x & 1) return i == dw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
    return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
  }
  const int r0 = y >> 1;
  int r1 = (y & 1) ? r0 + 1 : r0 - 1;
  r1 = r1 < 0 ? 0 : (r1 > dh - 1 ? dh - 1 : r1);
  const unsigned char *a = pl + (int64_t)r0 * pitch, *c = pl + (int64_t)r1 * pitch;
  const int s = 3 * a[i] + c[i];
  if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * a[i + 1] + c[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * a[i - 1] + c[i - 1] + 8) >> 4;
}

JD_HD void ycc_to_rgb(int Y, int Cb, int Cr, unsigned char* rgb) {
  const int cb = Cb - 128, cr = Cr - 128;
  rgb[0] = (unsigned char)clamp255(Y + ((91881 * cr + 32768) >> 16));
  rgb[1] = (unsigned char)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = (unsigned char)clamp255(Y + ((116130 * cb + 32768) >> 16));
}

}  // namespace jpegdec
#endif  // CODETR_JPEG_DEC_CORE_H_
