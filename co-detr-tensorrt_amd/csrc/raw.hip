// Raw Bayer frames on the GPU (include/codetr_raw.h states the rule): the colour-filter mosaic a sensor delivers -- one
// sample per pixel, 8 bits or a 16-bit container -- normalised, demosaiced (Malvar-He-Cutler 5 x 5 or bilinear 3 x 3) and
// toned into the packed RGB images every later kernel reads.  1 or 2 bytes read and 3 written per pixel; the arithmetic is
// a 5 x 5 integer stencil with four site types.
//
// raw_to_rgb_kernel<kBytes, kMethod>
//                     grid (ceil(Wmax / 64), ceil(Hmax / 64), N), 256 threads; the frame's table entry is a kernel argument
//                     read with a uniform index.  kBytes (1: uint8 samples, 2: the uint16 container) and the method are
//                     template parameters: four instances of one text.  A workgroup owns one T_w x T_h = 64 x 64 tile
//                     of OUTPUT pixels; tiles start at multiples of 64, so the parity of a tile-local coordinate is the
//                     parity of the image coordinate.
//   staging           The tile plus a halo of 2 samples, up to 68 x 68, goes to LDS as uint16 v of the rule's step 1:
//                     already folded at the borders (step 2) and normalised, so the 64-bit multiply runs once per sample
//                     and not once per tap, and the stencil below knows no border.  A thread stages groups of 4 samples
//                     (row r, columns 4 g .. 4 g + 3 of the staged window, 17 groups a row).  A group that lies inside
//                     the row is read as the 2 (kBytes = 1) or 3 (kBytes = 2) ALIGNED dwords that cover its 4 or 8 bytes,
//                     whatever the frame's byte offset and pitch, and funnel-shifted into place; the dwords are read only
//                     when they lie inside [src, src + src_bytes) -- bytes of a neighbouring row or of the gap between
//                     rows may be loaded and are dropped.  A group that crosses an image border, or whose dwords would
//                     leave the buffer, reads its samples one by one at their folded indices.  The multiplier of a sample
//                     is chosen from the pattern and the parities of its row and column with selects on uniform values.
//   LDS               uint16 sv[68][72] (9792 bytes) and the 4096-byte tone table: 13888 bytes, no large-LDS opt-in, and
//                     the 8 workgroups per CU that the wave limit allows still fit the default 64 KB.
//   stencil           A thread owns runs of 4 consecutive output pixels of one row (1024 runs a tile, 4 a thread).  With
//                     q = tid >> 4 (the 16-lane quarter, 0..15) and pass k = 0..3 the run is
//                       row r = (k & 1) + 2 (q >> 2) + 8 (q & 3) + 32 (k >> 1),   columns 4 (tid & 15) .. + 3:
//                     every row of the tile once, the four quarters of a wave on rows 8 apart, and the row parity k & 1
//                     a constant of the unrolled pass.  Runs start at even columns, so the parity of pixel i is i & 1.
//                     Site type therefore never diverges: whether even columns are green, and whether the row is a red
//                     row, are uniform values (pattern, k); the first picks one of two straight-line instances of the
//                     run's code with a uniform branch, the second is a select.  There is no per-pixel branch.
//                     The run reads its window -- 5 rows (3 for bilinear) of 8 samples, columns x - 2 .. x + 5 -- as two
//                     8-byte LDS reads per row, forms C, H1, V1, H2, V2, D of the header per pixel from registers,
//                     applies the two filters its site needs, looks the three channels up in the table (ds_read_u8) and
//                     stores 12 bytes as three dwords where the address is 4-byte aligned and the run is whole, byte by
//                     byte otherwise (ragged right edge, images whose 3 W is no multiple of 4, odd offsets).
//   LDS banks         Model (tests/test_lds_bank_model.py): 64 banks of 4 bytes, bank = dword address mod 64; an 8-byte
//                     read is served in two groups of 32 lanes; lanes of a group conflict when they touch different
//                     dwords of one bank.  Pitch: 72 samples = 36 dwords.
//                       window read (10 per run, the hot access): lane l reads dwords 36 (r + dy) + 2 (l & 15) + {0, 1}
//                         (+ 2 for the second read).  The 16 lanes of a quarter cover 32 consecutive dwords; the next
//                         quarter is 8 rows on, 288 dwords = 32 mod 64: the other 32 banks.  0 conflicts.  (With the
//                         quarters on the next rows of their parity -- 72 dwords apart -- 24 of the 32 banks would be hit
//                         twice; a pitch of 34 dwords, the window's own width, needs the quarters 16 rows apart.)
//                       staging write (4.5 per thread): lane of group index g writes dwords 2 g + 2 r + {0, 1}, r = g / 17:
//                         32 consecutive g cover 64 consecutive dwords but for the 2 dwords skipped at each row change, 1
//                         or 2 changes per 32 lanes: 2 or 4 banks are hit twice, the rest once.
//                       table reads are one byte at a data-dependent index: not modelled.
//   Nothing outside [src, src + src_bytes) is read, nothing outside an output image is written.  No scratch.
// A translation unit of its own on purpose: the code of frames.hip is pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_raw.h"
#include "raw_args.h"

namespace {

constexpr int kTile = 64;                  // output pixels per tile side (T_w = T_h)
constexpr int kHalo = 2;
constexpr int kPix = 4;                    // pixels per run, samples per staged group
constexpr int kThreads = 256;
constexpr int kSide = kTile + 2 * kHalo;   // staged rows and columns
constexpr int kGroups = kSide / kPix;      // staged groups per row
constexpr int kPitch = 72;                 // samples per LDS row (36 dwords: see "LDS banks")

struct FrameTable {  // a kernel argument, like frames.hip's FrameTable
  raw::Frame f[CODETR_PREPROCESS_BATCH_MAX];
};
struct Operands {
  unsigned black, white, m[3];
};

typedef unsigned u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ unsigned funnel(unsigned lo, unsigned hi, unsigned shift) {  // (hi:lo) >> shift, shift < 32
  return (unsigned)((((uint64_t)hi << 32) | lo) >> shift);
}

// the samples x .. x + 3 of a row of W (x even, possibly outside [0, W): folded), as the rule's s
template <int kBytes>
__device__ __forceinline__ void load_samples(const unsigned char* __restrict__ row, int x, int W, uintptr_t lo, uintptr_t hi,
                                             unsigned (&s)[kPix]) {
  constexpr int kWords = kBytes + 1;  // aligned dwords that cover 4 samples at any allowed address
  const uintptr_t p = (uintptr_t)(row + (int64_t)x * kBytes), a = p & ~(uintptr_t)3;
  if (x >= 0 && x + kPix <= W && a >= lo && a + 4 * kWords <= hi) {
    const unsigned* __restrict__ q = reinterpret_cast<const unsigned*>(a);
    const unsigned shift = 8u * (unsigned)(p & 3), w0 = q[0], w1 = q[1];
    if (kBytes == 1) {
      const unsigned v = funnel(w0, w1, shift);
#pragma unroll
      for (int i = 0; i < kPix; ++i) s[i] = (v >> (8 * i)) & 0xFFu;
    } else {
      const unsigned w2 = q[2], v0 = funnel(w0, w1, shift), v1 = funnel(w1, w2, shift);
      s[0] = v0 & 0xFFFFu, s[1] = v0 >> 16, s[2] = v1 & 0xFFFFu, s[3] = v1 >> 16;
    }
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const int xi = raw::fold(x + i, W);
      s[i] = kBytes == 1 ? row[xi] : (unsigned)row[2 * xi] | (unsigned)row[2 * xi + 1] << 8;
    }
  }
}

// step 1 of the rule
__device__ __forceinline__ unsigned normalise(unsigned s, unsigned m, const Operands& op) {
  s = min(s, op.white);
  const unsigned x = s > op.black ? s - op.black : 0u;
  const uint64_t t = ((uint64_t)x * m + 32768u) >> 16;
  return t > 65535u ? 65535u : (unsigned)t;
}

__device__ __forceinline__ int clamp16(int v) { return min(65535, max(0, v)); }

// One run: the window w[dy][c] (rows y - 2 .. y + 2, columns x - 2 .. x + 5 of the run at x) -> 4 pixels, one dword each
// (R | G << 8 | B << 16).  kEvenGreen: the run's even pixels are green sites; red_row: the row holds the red sites.
template <int kMethod, bool kEvenGreen>
__device__ __forceinline__ void demosaic_run(const int (&w)[5][kPix + 4], bool red_row, const unsigned char* __restrict__ lut,
                                             unsigned (&px)[kPix]) {
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    const bool green = kEvenGreen != ((i & 1) != 0);
    const int c = i + kHalo;
    const int C = w[2][c], H1 = w[2][c - 1] + w[2][c + 1], V1 = w[1][c] + w[3][c];
    const int D = w[1][c - 1] + w[1][c + 1] + w[3][c - 1] + w[3][c + 1];
    int a, b;  // green site: the colour of the row, the other one; red / blue site: green, the opposite colour
    if (kMethod == CODETR_RAW_MALVAR) {
      const int H2 = w[2][c - 2] + w[2][c + 2], V2 = w[0][c] + w[4][c];
      if (green) {
        a = clamp16((10 * C + 8 * H1 - 2 * H2 + V2 - 2 * D + 8) >> 4);
        b = clamp16((10 * C + 8 * V1 - 2 * V2 + H2 - 2 * D + 8) >> 4);
      } else {
        a = clamp16((8 * C + 4 * (H1 + V1) - 2 * (H2 + V2) + 8) >> 4);
        b = clamp16((12 * C + 4 * D - 3 * (H2 + V2) + 8) >> 4);
      }
    } else {
      a = green ? (H1 + 1) >> 1 : (H1 + V1 + 2) >> 2;
      b = green ? (V1 + 1) >> 1 : (D + 2) >> 2;
    }
    const int R = green ? (red_row ? a : b) : (red_row ? C : b);
    const int G = green ? C : a;
    const int B = green ? (red_row ? b : a) : (red_row ? b : C);
    px[i] = (unsigned)lut[R >> 4] | (unsigned)lut[G >> 4] << 8 | (unsigned)lut[B >> 4] << 16;
  }
}

// npx (1..4) pixels, one dword each (the top byte zero) -> 3 npx bytes at q
__device__ __forceinline__ void store_run(unsigned char* __restrict__ q, int npx, const unsigned (&px)[kPix]) {
  if (npx == kPix && ((uintptr_t)q & 3u) == 0) {
    u32x3_a4 o;
    o.x = px[0] | px[1] << 24;
    o.y = px[1] >> 8 | px[2] << 16;
    o.z = px[2] >> 16 | px[3] << 8;
    *reinterpret_cast<u32x3_a4*>(q) = o;
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      if (i < npx) {
        q[3 * i] = (unsigned char)px[i];
        q[3 * i + 1] = (unsigned char)(px[i] >> 8);
        q[3 * i + 2] = (unsigned char)(px[i] >> 16);
      }
    }
  }
}

// grid (ceil(Wmax / 64), ceil(Hmax / 64), N)
template <int kBytes, int kMethod>
__global__ __launch_bounds__(kThreads) void raw_to_rgb_kernel(const unsigned char* __restrict__ src, int64_t src_bytes,
                                                              FrameTable tab, Operands op, const uint4* __restrict__ lut,
                                                              unsigned char* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) unsigned short sv[kSide * kPitch];
  __shared__ __attribute__((aligned(16))) unsigned char slut[CODETR_RAW_LUT_BYTES];
  const raw::Frame& im = tab.f[blockIdx.z];  // (uniform: the entry comes through the scalar cache)
  const int H = im.H, W = im.W;
  const int ty = blockIdx.y * kTile, tx = blockIdx.x * kTile;
  if (ty >= H || tx >= W) return;  // (uniform)
  const int nr = min(kTile, H - ty), nc = min(kTile, W - tx);  // output rows and columns of this tile
  reinterpret_cast<uint4*>(slut)[threadIdx.x] = lut[threadIdx.x];  // 256 x 16 bytes

  // staged rows 0 .. nr + 3 are image rows ty - 2 ..; staged groups 0 .. ng - 1 cover the columns tx - 2 .. tx + nc + 1
  const int ng = (nc + 2 * kHalo + kPix - 1) / kPix;
  const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)src_bytes;
  const unsigned char* __restrict__ s = src + im.src;
  const bool rx0 = im.rx == 0;
  for (int g = threadIdx.x; g < (nr + 2 * kHalo) * kGroups; g += kThreads) {
    const int r = g / kGroups, cg = g - r * kGroups;
    if (cg >= ng) continue;
    unsigned smp[kPix];
    load_samples<kBytes>(s + (int64_t)raw::fold(ty - kHalo + r, H) * im.pitch, tx - kHalo + kPix * cg, W, lo, hi, smp);
    // ty - 2 and tx - 2 are even and the fold keeps parities: the staged row and column parities are those of the sample's
    // own site -- but on an axis of length 1, where every index reads sample 0.  A red row holds red at column parity rx
    // and green beside it; a blue row blue at parity 1 - rx.
    const bool red_row = (H == 1 ? 0 : r & 1) == im.ry;
    const unsigned m_even = red_row ? (rx0 ? op.m[0] : op.m[1]) : (rx0 ? op.m[1] : op.m[2]);
    const unsigned m_odd = W == 1 ? m_even : red_row ? (rx0 ? op.m[1] : op.m[0]) : (rx0 ? op.m[2] : op.m[1]);
    uint2 v;
    v.x = normalise(smp[0], m_even, op) | normalise(smp[1], m_odd, op) << 16;
    v.y = normalise(smp[2], m_even, op) | normalise(smp[3], m_odd, op) << 16;
    *reinterpret_cast<uint2*>(&sv[r * kPitch + kPix * cg]) = v;
  }
  __syncthreads();

  unsigned char* __restrict__ d = dst + im.dst;
  const int q = threadIdx.x >> 4, col = (threadIdx.x & 15) * kPix;
  const int rbase = 2 * (q >> 2) + 8 * (q & 3);
  constexpr int kFirst = kMethod == CODETR_RAW_MALVAR ? 0 : 1, kLast = kMethod == CODETR_RAW_MALVAR ? 4 : 3;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = (k & 1) + rbase + 32 * (k >> 1);
    if (r >= nr || col >= nc) continue;
    int w[5][kPix + 4] = {};
#pragma unroll
    for (int dy = kFirst; dy <= kLast; ++dy) {  // staged row r + dy is image row ty + r + dy - 2; staged column col is x - 2
      const uint2* __restrict__ p = reinterpret_cast<const uint2*>(&sv[(r + dy) * kPitch + col]);
      const uint2 lo2 = p[0], hi2 = p[1];
      w[dy][0] = lo2.x & 0xFFFFu, w[dy][1] = lo2.x >> 16, w[dy][2] = lo2.y & 0xFFFFu, w[dy][3] = lo2.y >> 16;
      w[dy][4] = hi2.x & 0xFFFFu, w[dy][5] = hi2.x >> 16, w[dy][6] = hi2.y & 0xFFFFu, w[dy][7] = hi2.y >> 16;
    }
    const bool red_row = (k & 1) == im.ry;
    unsigned px[kPix];
    if (((k & 1) ^ im.ry ^ im.rx) != 0) {  // (uniform) a site is green when its parities differ from the red site's in one axis
      demosaic_run<kMethod, true>(w, red_row, slut, px);
    } else {
      demosaic_run<kMethod, false>(w, red_row, slut, px);
    }
    store_run(d + ((int64_t)(ty + r) * W + tx + col) * 3, min(kPix, nc - col), px);
  }
}

template <int kBytes, int kMethod>
void launch(hipStream_t stream, const dim3& grid, const void* src, int64_t src_bytes, const FrameTable& tab, const Operands& op,
            const void* lut, void* dst) {
  hipLaunchKernelGGL((raw_to_rgb_kernel<kBytes, kMethod>), grid, dim3(kThreads), 0, stream, static_cast<const unsigned char*>(src),
                     src_bytes, tab, op, static_cast<const uint4*>(lut), static_cast<unsigned char*>(dst));
}

}  // namespace

extern "C" int codetr_raw_abi_version(void) { return CODETR_RAW_ABI_VERSION; }

extern "C" int codetr_raw_multipliers(int64_t black, int64_t white, const double* gains_host, int64_t* m_host) {
  if (!gains_host || !m_host) return CODETR_E_BADARG;
  return raw::multipliers(black, white, gains_host, m_host) ? 0 : CODETR_E_BADARG;
}

extern "C" int codetr_raw_to_rgb_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host,
                                    const int64_t* settings_host, const void* lut_dev, void* dst_dev, int64_t dst_bytes) {
  raw::Checked c;
  const int rc = raw::check((uintptr_t)src_dev, src_bytes, N, rows_host, settings_host, (uintptr_t)lut_dev, (uintptr_t)dst_dev,
                            dst_bytes, &c);
  if (rc != 0) return rc;
  FrameTable tab = {};
  for (int64_t n = 0; n < N; ++n) tab.f[n] = c.f[n];
  const Operands op = {c.black, c.white, {c.m[0], c.m[1], c.m[2]}};
  const dim3 grid((unsigned)((c.Wmax + kTile - 1) / kTile), (unsigned)((c.Hmax + kTile - 1) / kTile), (unsigned)N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (c.bytes == 1) {
    if (c.method == CODETR_RAW_MALVAR) launch<1, CODETR_RAW_MALVAR>(st, grid, src_dev, src_bytes, tab, op, lut_dev, dst_dev);
    else launch<1, CODETR_RAW_BILINEAR>(st, grid, src_dev, src_bytes, tab, op, lut_dev, dst_dev);
  } else {
    if (c.method == CODETR_RAW_MALVAR) launch<2, CODETR_RAW_MALVAR>(st, grid, src_dev, src_bytes, tab, op, lut_dev, dst_dev);
    else launch<2, CODETR_RAW_BILINEAR>(st, grid, src_dev, src_bytes, tab, op, lut_dev, dst_dev);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}
