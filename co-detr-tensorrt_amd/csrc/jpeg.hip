// Baseline JPEG encoder for the RGB images the drawing and frame kernels leave on the device (include/codetr_jpeg.h states
// the file and every rounding; tests/jpeg_ref.py restates it in numpy and the GPU tests compare byte for byte).
//
// Two launches, no host synchronisation:
//   jpeg_encode_rows_kernel   one 256-thread workgroup per MCU row (= one restart interval).  The row is encoded in passes
//     of kPassPixels pixels = 168 blocks: (0) the workgroup converts the pass's pixels to Y / Cb / Cr samples in LDS
//     (coalesced along x, edge pixels repeated); (A) one thread per block runs the integer DCT in registers, quantises
//     with a reciprocal multiply and leaves the 64 zigzag coefficients in LDS, coefficient-major (lane = block: no bank
//     conflict); (B) the thread counts its block's bits, a workgroup scan turns the counts into bit offsets; (C) it
//     writes its codes with atomicOr into a zeroed LDS bit buffer that aliases the samples; (D) every thread takes an
//     equal share of the pass's whole bytes, a second scan over its FF count places them, and the bytes (each FF followed
//     by 00) go to the row's slice of the workspace.  The incomplete last byte, the three DC predictors and the row's
//     byte count travel to the next pass in registers.
//   jpeg_gather_rows_kernel   one workgroup per MCU row again: it sums the row lengths of its image (at most 2048), so it
//     knows its own offset and whether the image fits its slot, and copies its row and RST marker there.
// LDS: 21 504 (coefficients) + 34 872 (bit buffer: 168 blocks x 1660 bits, the proven bound of a block) + 2 176 (code
// tables) + 512 (quantiser) + scans < 64 KB, all static.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "codetr_jpeg.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPassPixels = CODETR_JPEG_PASS_PIXELS;
constexpr int kMaxBlocks = 168;                       // 28 MCUs x 6 blocks at 4:2:0, 56 x 3 at 4:4:4
constexpr int kBlockBits = 1660;                      // 22 (DC) + 63 x 26 (AC): the most bits one block can take
constexpr int kBitWords = (kMaxBlocks * kBlockBits + 7 + 31) / 32 + 1;   // + the carried bits, + the spill word of a put
constexpr int kSampleStride = 68;                     // bytes per block of samples: 17 dwords, conflict-free dword reads
static_assert(kPassPixels / 16 * 6 == kMaxBlocks && kPassPixels / 8 * 3 == kMaxBlocks, "pass size");
static_assert(kMaxBlocks * kSampleStride <= kBitWords * 4, "the samples alias the bit buffer");
static_assert(CODETR_JPEG_BLOCK_BOUND == 2 * ((kBlockBits + 7) / 8), "block bound");

constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.1 / K.2, natural order
constexpr unsigned char kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// T.81 Annex K.3 - K.6: codes per length 1..16, then the symbols in code order.  Index: 0 DC lum, 1 AC lum, 2 DC chrom,
// 3 AC chrom (the order of the DHT segments).
struct HuffSpec {
  unsigned char bits[16];
  int count;
  unsigned char vals[162];
};
constexpr HuffSpec kHuff[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
     162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}};

// symbol -> (code << 5) | length; 0 for a symbol the table does not hold
struct HuffLut {
  unsigned v[256];
};
constexpr HuffLut build_lut(const HuffSpec& h) {
  HuffLut l = {};
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < h.bits[len - 1]; ++i) l.v[h.vals[k++]] = (code++ << 5) | (unsigned)len;
    code <<= 1;
  }
  return l;
}
__constant__ const HuffLut d_lut[4] = {build_lut(kHuff[0]), build_lut(kHuff[1]), build_lut(kHuff[2]), build_lut(kHuff[3])};

struct JpegImage {
  int64_t offset;   // of the image in buf
  int64_t ws_off;   // of its first row's bytes in the workspace
  int H, W;
  int rows, mcus;   // MCU rows, MCUs per row
  int row0;         // index of its first row among all rows of the call (= the workgroup index)
  int rowcap;       // bytes a row may take in the workspace
  int rowstride;    // rowcap rounded up to 16
  int pad_;
};
struct JpegTable {
  JpegImage img[CODETR_PREPROCESS_BATCH_MAX];
};
// per zigzag position: (m << 8) | t with m = 2^20 / t + 1, so that a / t == (a * m) >> 20 for every a < 4096
// (a * (m t - 2^20) <= 4095 * 255 < 2^20); a = |F| + t / 2 <= 1024 + 127.  [0]: luminance, [1]: chrominance.
struct JpegQuant {
  unsigned q[2][64];
};

// exclusive scan of one int per thread over the 256-thread workgroup; every thread calls it
__device__ __forceinline__ int block_scan_excl(int v, int* s_wave, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();   // (the previous scan's totals have been read)
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kThreads / 64; ++i) {
    const int t = s_wave[i];
    base += i < w ? t : 0;
    total += t;
  }
  return base + inc - v;
}

// in-place 8-point DCT of v[0], v[S], ..., v[7 S] by the matrix of the header, (sum + RND) >> SH.  The even / odd split
// uses C[k][7 - n] = (-1)^k C[k][n]: the same integer sums in another order, so the result is the stated one.
template <int S, int RND, int SH>
__device__ __forceinline__ void dct8(int* v) {
  const int a0 = v[0] + v[7 * S], a1 = v[S] + v[6 * S], a2 = v[2 * S] + v[5 * S], a3 = v[3 * S] + v[4 * S];
  const int b0 = v[0] - v[7 * S], b1 = v[S] - v[6 * S], b2 = v[2 * S] - v[5 * S], b3 = v[3 * S] - v[4 * S];
  v[0] = (2896 * (a0 + a1 + a2 + a3) + RND) >> SH;
  v[4 * S] = (2896 * (a0 - a1 - a2 + a3) + RND) >> SH;
  v[2 * S] = (3784 * (a0 - a3) + 1567 * (a1 - a2) + RND) >> SH;
  v[6 * S] = (1567 * (a0 - a3) - 3784 * (a1 - a2) + RND) >> SH;
  v[S] = (4017 * b0 + 3406 * b1 + 2276 * b2 + 799 * b3 + RND) >> SH;
  v[3 * S] = (3406 * b0 - 799 * b1 - 4017 * b2 - 2276 * b3 + RND) >> SH;
  v[5 * S] = (2276 * b0 - 4017 * b1 + 799 * b2 + 3406 * b3 + RND) >> SH;
  v[7 * S] = (799 * b0 - 2276 * b1 + 3406 * b2 - 4017 * b3 + RND) >> SH;
}

__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v < 0 ? -v : v); }   // 0 for 0

// `len` <= 26 bits of `val` at bit `pos` of the buffer (bit 0 = the top bit of word 0); the words were zeroed
__device__ __forceinline__ void put_bits(unsigned* s_bits, int pos, unsigned val, int len) {
  const unsigned long long w = (unsigned long long)val << (64 - (pos & 31) - len);
  atomicOr(&s_bits[pos >> 5], (unsigned)(w >> 32));
  if ((unsigned)w) atomicOr(&s_bits[(pos >> 5) + 1], (unsigned)w);
}

__device__ __forceinline__ void rgb_to_ycc(const unsigned char* p, int& y, int& cb, int& cr) {
  const int r = p[0], g = p[1], b = p[2];
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = min((-11058 * r - 21710 * g + 32768 * b + 8388608 + 32768) >> 16, 255);
  cr = min((32768 * r - 27439 * g - 5329 * b + 8388608 + 32768) >> 16, 255);
}

template <bool k444>
__global__ __launch_bounds__(kThreads) void jpeg_encode_rows_kernel(const unsigned char* __restrict__ buf, JpegTable tab,
                                                                    JpegQuant quant, int N, unsigned char* __restrict__ ws) {
  constexpr int kBpm = k444 ? 3 : 6;              // blocks per MCU
  constexpr int kMcuPx = k444 ? 8 : 16;
  constexpr int kPassMcus = kPassPixels / kMcuPx;
  __shared__ short s_coef[64 * kMaxBlocks];
  __shared__ unsigned s_bits[kBitWords];
  __shared__ unsigned s_ac[2][256];
  __shared__ unsigned s_dc[2][16];
  __shared__ unsigned s_q[2][64];
  __shared__ int s_wave[kThreads / 64];
  unsigned char* const s_smp = reinterpret_cast<unsigned char*>(s_bits);

  const int tid = threadIdx.x;
  int n = 0;
  while (n + 1 < N && (int)blockIdx.x >= tab.img[n + 1].row0) ++n;
  const JpegImage im = tab.img[n];
  const int r = (int)blockIdx.x - im.row0;
  const unsigned char* const img = buf + im.offset;
  const int H = im.H, W = im.W;
  const int y0 = r * kMcuPx;

  for (int i = tid; i < 512; i += kThreads) s_ac[i >> 8][i & 255] = d_lut[1 + 2 * (i >> 8)].v[i & 255];
  if (tid < 32) s_dc[tid >> 4][tid & 15] = d_lut[2 * (tid >> 4)].v[tid & 15];
  if (tid < 128) s_q[tid >> 6][tid & 63] = quant.q[tid >> 6][tid & 63];

  // what a pass hands to the next
  int carry_bits = 0;        // bits of the incomplete last byte
  unsigned carry_byte = 0;   // that byte, its bits at the top
  int dcprev_y = 0, dcprev_cb = 0, dcprev_cr = 0;
  int rowbytes = 0;
  bool overflow = false;
  unsigned char* const dst = ws + im.ws_off + (int64_t)r * im.rowstride;

  for (int m0 = 0; m0 < im.mcus; m0 += kPassMcus) {
    const int Mp = min(kPassMcus, im.mcus - m0);
    const int nblk = Mp * kBpm;
    const bool last = m0 + kPassMcus >= im.mcus;

    // ---- (0) pixels -> samples
    if (k444) {
      const int wpx = Mp * 8;
      for (int i = tid; i < wpx * 8; i += kThreads) {
        const int py = i / wpx, px = i - py * wpx;
        const int x = min(m0 * 8 + px, W - 1), y = min(y0 + py, H - 1);
        int yy, cb, cr;
        rgb_to_ycc(img + ((size_t)y * W + x) * 3, yy, cb, cr);
        unsigned char* o = s_smp + (px >> 3) * 3 * kSampleStride + py * 8 + (px & 7);
        o[0] = (unsigned char)yy;
        o[kSampleStride] = (unsigned char)cb;
        o[2 * kSampleStride] = (unsigned char)cr;
      }
    } else {
      const int wq = Mp * 8;   // quads (2x2 pixels) per quad row
      for (int i = tid; i < wq * 8; i += kThreads) {
        const int qy = i / wq, qx = i - qy * wq;
        const int xa = min(m0 * 16 + 2 * qx, W - 1), xb = min(m0 * 16 + 2 * qx + 1, W - 1);
        const int ya = min(y0 + 2 * qy, H - 1), yb = min(y0 + 2 * qy + 1, H - 1);
        int yy[4], cb[4], cr[4];
        rgb_to_ycc(img + ((size_t)ya * W + xa) * 3, yy[0], cb[0], cr[0]);
        rgb_to_ycc(img + ((size_t)ya * W + xb) * 3, yy[1], cb[1], cr[1]);
        rgb_to_ycc(img + ((size_t)yb * W + xa) * 3, yy[2], cb[2], cr[2]);
        rgb_to_ycc(img + ((size_t)yb * W + xb) * 3, yy[3], cb[3], cr[3]);
        const int m = qx >> 3, lx = (qx & 7) * 2, ly = qy * 2;   // lx, lx + 1 (ly, ly + 1) lie in one block
        unsigned char* o = s_smp + (m * 6 + ((ly >> 3) << 1) + (lx >> 3)) * kSampleStride + (ly & 7) * 8 + (lx & 7);
        o[0] = (unsigned char)yy[0];
        o[1] = (unsigned char)yy[1];
        o[8] = (unsigned char)yy[2];
        o[9] = (unsigned char)yy[3];
        unsigned char* c = s_smp + (m * 6 + 4) * kSampleStride + qy * 8 + (qx & 7);
        c[0] = (unsigned char)((cb[0] + cb[1] + cb[2] + cb[3] + 2) >> 2);
        c[kSampleStride] = (unsigned char)((cr[0] + cr[1] + cr[2] + cr[3] + 2) >> 2);
      }
    }
    __syncthreads();

    // ---- (A) DCT + quantisation, one thread per block
    const int sub = tid % kBpm;                                 // position of the block in its MCU
    const int comp = k444 ? sub : (sub < 4 ? 0 : sub - 3);      // 0 Y, 1 Cb, 2 Cr
    const int ti = comp ? 1 : 0;                                // table set
    if (tid < nblk) {
      int d[64];
      const unsigned* sp = reinterpret_cast<const unsigned*>(s_smp + tid * kSampleStride);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned w = sp[i];
        d[4 * i] = (int)(w & 255u) - 128;
        d[4 * i + 1] = (int)((w >> 8) & 255u) - 128;
        d[4 * i + 2] = (int)((w >> 16) & 255u) - 128;
        d[4 * i + 3] = (int)(w >> 24) - 128;
      }
#pragma unroll
      for (int y = 0; y < 8; ++y) dct8<1, 512, 10>(d + 8 * y);
#pragma unroll
      for (int x = 0; x < 8; ++x) dct8<8, 32768, 16>(d + x);
#pragma unroll
      for (int k = 0; k < 64; ++k) {
        const int c = d[kZigzag[k]];
        const unsigned q = s_q[ti][k];
        const int t = (int)(q & 255u);
        const int a = (int)((((unsigned)(c < 0 ? -c : c) + (unsigned)(t >> 1)) * (q >> 8)) >> 20);
        s_coef[k * kMaxBlocks + tid] = (short)(c < 0 ? -a : a);
      }
    }
    __syncthreads();   // the samples are dead from here: s_bits is the bit buffer

    // ---- (B) bits per block -> bit offsets
    int diff = 0, nbits = 0;
    if (tid < nblk) {
      // previous block of the component: Y1..Y3 follow their neighbour, Y0 the last MCU's Y3; chroma the last MCU's
      const int pb = k444 ? tid - 3 : (sub == 0 ? tid - 3 : sub < 4 ? tid - 1 : tid - 6);
      diff = (int)s_coef[tid] - (pb >= 0 ? (int)s_coef[pb] : comp == 0 ? dcprev_y : comp == 1 ? dcprev_cb : dcprev_cr);
      const int cat = bit_length(diff);
      nbits = (int)(s_dc[ti][cat] & 31u) + cat;
      const int zrl = (int)(s_ac[ti][0xF0] & 31u);
      int run = 0;
      for (int k = 1; k < 64; ++k) {
        const int v = s_coef[k * kMaxBlocks + tid];
        if (v == 0) {
          ++run;
        } else {
          nbits += (run >> 4) * zrl;
          const int sz = bit_length(v);
          nbits += (int)(s_ac[ti][((run & 15) << 4) | sz] & 31u) + sz;
          run = 0;
        }
      }
      if (run) nbits += (int)(s_ac[ti][0] & 31u);
    }
    int total;
    const int off = block_scan_excl(nbits, s_wave, total);
    const int endbit = carry_bits + total;
    const int nwords = (endbit + 31) / 32 + 1;   // <= kBitWords
    for (int i = tid; i < nwords; i += kThreads) s_bits[i] = i == 0 ? carry_byte << 24 : 0u;
    __syncthreads();

    // ---- (C) the codes
    if (tid < nblk) {
      int pos = carry_bits + off;
      {
        const int cat = bit_length(diff);
        const unsigned e = s_dc[ti][cat];
        const unsigned mag = (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u);
        put_bits(s_bits, pos, ((e >> 5) << cat) | mag, (int)(e & 31u) + cat);
        pos += (int)(e & 31u) + cat;
      }
      const unsigned zrl = s_ac[ti][0xF0];
      int run = 0;
      for (int k = 1; k < 64; ++k) {
        const int v = s_coef[k * kMaxBlocks + tid];
        if (v == 0) {
          ++run;
        } else {
          for (; run >= 16; run -= 16) {
            put_bits(s_bits, pos, zrl >> 5, (int)(zrl & 31u));
            pos += (int)(zrl & 31u);
          }
          const int sz = bit_length(v);
          const unsigned e = s_ac[ti][(run << 4) | sz];
          const unsigned mag = (unsigned)(v < 0 ? v - 1 : v) & ((1u << sz) - 1u);
          put_bits(s_bits, pos, ((e >> 5) << sz) | mag, (int)(e & 31u) + sz);
          pos += (int)(e & 31u) + sz;
          run = 0;
        }
      }
      if (run) {
        const unsigned e = s_ac[ti][0];
        put_bits(s_bits, pos, e >> 5, (int)(e & 31u));
      }
    }
    const int pad = last ? (-endbit) & 7 : 0;   // the row's tail: 1-bits up to a byte
    if (pad && tid == 0) put_bits(s_bits, endbit, (1u << pad) - 1u, pad);
    __syncthreads();

    // ---- (D) whole bytes -> the workspace, FF followed by 00
    const int nbytes = (endbit + pad) >> 3;
    const int per = (nbytes + kThreads - 1) / kThreads;
    const int b0 = min(tid * per, nbytes), b1 = min(b0 + per, nbytes);
    int ff = 0;
    for (int i = b0; i < b1; ++i) ff += ((s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
    int totff;
    const int ffoff = block_scan_excl(ff, s_wave, totff);
    if (rowbytes + nbytes + totff > im.rowcap) overflow = true;   // (uniform: every thread holds the same totals)
    if (!overflow) {
      unsigned char* o = dst + rowbytes + b0 + ffoff;
      for (int i = b0; i < b1; ++i) {
        const unsigned v = (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
        *o++ = (unsigned char)v;
        if (v == 255u) *o++ = 0;
      }
    }
    rowbytes += nbytes + totff;
    carry_bits = endbit & 7;
    carry_byte = last ? 0u : (s_bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u;
    dcprev_y = s_coef[nblk - kBpm + (k444 ? 0 : 3)];
    dcprev_cb = s_coef[nblk - 2];
    dcprev_cr = s_coef[nblk - 1];
    __syncthreads();   // before the next pass writes samples over the bit buffer and new coefficients
  }
  if (tid == 0) reinterpret_cast<int*>(ws)[blockIdx.x] = overflow ? -1 : rowbytes;
}

__global__ __launch_bounds__(kThreads) void jpeg_gather_rows_kernel(JpegTable tab, int N, const unsigned char* __restrict__ ws,
                                                                    unsigned char* __restrict__ out, int64_t out_stride,
                                                                    int* __restrict__ lengths) {
  __shared__ long long s_sum[2][kThreads / 64];
  __shared__ int s_bad[kThreads / 64];
  const int tid = threadIdx.x;
  int n = 0;
  while (n + 1 < N && (int)blockIdx.x >= tab.img[n + 1].row0) ++n;
  const JpegImage im = tab.img[n];
  const int r = (int)blockIdx.x - im.row0;
  const int* lens = reinterpret_cast<const int*>(ws) + im.row0;
  long long before = 0, total = 0;
  int bad = 0;
  for (int j = tid; j < im.rows; j += kThreads) {
    const int l = lens[j];
    bad |= l < 0;
    total += l;
    before += j < r ? l : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    before += __shfl_xor(before, d, 64);
    total += __shfl_xor(total, d, 64);
    bad |= __shfl_xor(bad, d, 64);
  }
  if ((tid & 63) == 0) s_sum[0][tid >> 6] = before, s_sum[1][tid >> 6] = total, s_bad[tid >> 6] = bad;
  __syncthreads();
  before = total = 0, bad = 0;
#pragma unroll
  for (int i = 0; i < kThreads / 64; ++i) before += s_sum[0][i], total += s_sum[1][i], bad |= s_bad[i];
  total += 2 * (long long)(im.rows - 1);   // the RST markers
  before += 2 * (long long)r;
  const bool fits = !bad && total <= out_stride;
  if (r == 0 && tid == 0) lengths[n] = fits ? (int)total : -1;
  if (!fits) return;
  const unsigned char* src = ws + im.ws_off + (int64_t)r * im.rowstride;
  unsigned char* dst = out + (int64_t)n * out_stride + before;
  const int len = lens[r];
  for (int i = tid; i < len; i += kThreads) dst[i] = src[i];
  if (r + 1 < im.rows && tid == 0) {
    dst[len] = 0xFF;
    dst[len + 1] = (unsigned char)(0xD0 + (r & 7));
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

int quant_table(int quality, int which, unsigned char* zigzag_out) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int k = 0; k < 64; ++k) {
    int t = (kBaseQuant[which][kZigzag[k]] * s + 50) / 100;
    zigzag_out[k] = (unsigned char)(t < 1 ? 1 : t > 255 ? 255 : t);
  }
  return 0;
}

bool bad_sub(int subsampling) { return subsampling != CODETR_JPEG_420 && subsampling != CODETR_JPEG_444; }

// the row table of a call and the bytes of its workspace; a CODETR_E_* code for rows the header rules out
int64_t plan(int64_t N, const int64_t* images, int subsampling, int64_t out_stride, int64_t buf_bytes, JpegTable* tab,
             int* total_rows) {
  if (!images || N <= 0 || out_stride <= 0 || bad_sub(subsampling)) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  const int px = subsampling == CODETR_JPEG_444 ? 8 : 16, bpm = subsampling == CODETR_JPEG_444 ? 3 : 6;
  int64_t rows = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t off = images[3 * n], H = images[3 * n + 1], W = images[3 * n + 2];
    if (off < 0 || H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_DRAW_MAX_SIDE || W > CODETR_DRAW_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (buf_bytes >= 0 && (off > buf_bytes || H * W * 3 > buf_bytes - off)) return CODETR_E_BADARG;
    rows += (H + px - 1) / px;
  }
  int64_t bytes = (rows * 4 + 15) / 16 * 16;
  int row0 = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t H = images[3 * n + 1], W = images[3 * n + 2];
    const int64_t mcus = (W + px - 1) / px, r = (H + px - 1) / px;
    const int64_t worst = mcus * bpm * CODETR_JPEG_BLOCK_BOUND;
    const int64_t cap = worst < out_stride ? worst : out_stride, stride = (cap + 15) / 16 * 16;
    if (tab) tab->img[n] = JpegImage{images[3 * n], bytes, (int)H, (int)W, (int)r, (int)mcus, row0, (int)cap, (int)stride, 0};
    bytes += r * stride;
    row0 += (int)r;
  }
  if (total_rows) *total_rows = row0;
  return bytes;
}

void put16(unsigned char*& p, int v) {
  *p++ = (unsigned char)(v >> 8);
  *p++ = (unsigned char)(v & 255);
}

}  // namespace

extern "C" {

int codetr_jpeg_abi_version(void) { return CODETR_JPEG_ABI_VERSION; }

int codetr_jpeg_header(int64_t H, int64_t W, int quality, int subsampling, unsigned char* out_host, int64_t capacity) {
  if (!out_host || H < 1 || W < 1 || H > 65535 || W > 65535 || quality < 1 || quality > 100 || bad_sub(subsampling) ||
      capacity < CODETR_JPEG_HEADER_BYTES)
    return CODETR_E_BADARG;
  unsigned char* p = out_host;
  put16(p, 0xFFD8);
  put16(p, 0xFFE0);
  put16(p, 16);
  memcpy(p, "JFIF\0\1\1\0\0\1\0\1\0\0", 14);
  p += 14;
  for (int i = 0; i < 2; ++i) {
    put16(p, 0xFFDB);
    put16(p, 67);
    *p++ = (unsigned char)i;
    quant_table(quality, i, p);
    p += 64;
  }
  put16(p, 0xFFC0);
  put16(p, 17);
  *p++ = 8;
  put16(p, (int)H);
  put16(p, (int)W);
  *p++ = 3;
  const unsigned char comps[9] = {1, (unsigned char)(subsampling == CODETR_JPEG_420 ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1};
  memcpy(p, comps, 9);
  p += 9;
  const unsigned char ids[4] = {0x00, 0x10, 0x01, 0x11};   // class << 4 | table
  for (int i = 0; i < 4; ++i) {
    put16(p, 0xFFC4);
    put16(p, 19 + kHuff[i].count);
    *p++ = ids[i];
    memcpy(p, kHuff[i].bits, 16);
    p += 16;
    memcpy(p, kHuff[i].vals, (size_t)kHuff[i].count);
    p += kHuff[i].count;
  }
  const int px = subsampling == CODETR_JPEG_444 ? 8 : 16;
  put16(p, 0xFFDD);
  put16(p, 4);
  put16(p, (int)((W + px - 1) / px));
  put16(p, 0xFFDA);
  put16(p, 12);
  const unsigned char sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  memcpy(p, sos, 10);
  p += 10;
  return (int)(p - out_host);
}

int64_t codetr_jpeg_scan_bound(int64_t H, int64_t W, int subsampling) {
  if (H < 1 || W < 1 || bad_sub(subsampling)) return CODETR_E_BADARG;
  if (H > CODETR_DRAW_MAX_SIDE || W > CODETR_DRAW_MAX_SIDE) return CODETR_E_TOO_LARGE;
  const int px = subsampling == CODETR_JPEG_444 ? 8 : 16, bpm = subsampling == CODETR_JPEG_444 ? 3 : 6;
  const int64_t rows = (H + px - 1) / px, mcus = (W + px - 1) / px;
  return rows * mcus * bpm * CODETR_JPEG_BLOCK_BOUND + 2 * (rows - 1);
}

int64_t codetr_jpeg_workspace_bytes(int64_t N, const int64_t* images_host, int subsampling, int64_t out_stride) {
  return plan(N, images_host, subsampling, out_stride, -1, nullptr, nullptr);
}

int codetr_jpeg_encode_u8(void* stream, const void* buf_dev, int64_t buf_bytes, int64_t N, const int64_t* images_host,
                          int quality, int subsampling, void* out_dev, int64_t out_stride, int* lengths_dev,
                          void* workspace_dev, int64_t workspace_bytes) {
  if (!buf_dev || !images_host || !out_dev || !lengths_dev || !workspace_dev || buf_bytes <= 0 || quality < 1 ||
      quality > 100)
    return CODETR_E_BADARG;
  JpegTable tab = {};
  int rows = 0;
  const int64_t need = plan(N, images_host, subsampling, out_stride, buf_bytes, &tab, &rows);
  if (need < 0) return (int)need;
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace_dev) & 15u)) return CODETR_E_BADARG;
  JpegQuant quant;
  for (int i = 0; i < 2; ++i) {
    unsigned char t[64];
    quant_table(quality, i, t);
    for (int k = 0; k < 64; ++k) quant.q[i][k] = (((1u << 20) / t[k] + 1u) << 8) | t[k];
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
  if (subsampling == CODETR_JPEG_444)
    hipLaunchKernelGGL(jpeg_encode_rows_kernel<true>, dim3((unsigned)rows), dim3(kThreads), 0, s,
                       static_cast<const unsigned char*>(buf_dev), tab, quant, (int)N, ws);
  else
    hipLaunchKernelGGL(jpeg_encode_rows_kernel<false>, dim3((unsigned)rows), dim3(kThreads), 0, s,
                       static_cast<const unsigned char*>(buf_dev), tab, quant, (int)N, ws);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(jpeg_gather_rows_kernel, dim3((unsigned)rows), dim3(kThreads), 0, s, tab, (int)N, ws,
                     static_cast<unsigned char*>(out_dev), out_stride, lengths_dev);
  err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // extern "C"
