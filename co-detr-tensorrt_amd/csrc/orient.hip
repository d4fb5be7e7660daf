// EXIF orientations on the GPU (include/codetr_orient.h states the rule): the stored packed RGB images of a chunk -- what
// frames_to_rgb_kernel and the JPEG decoder leave -- written once more as the upright images every later kernel reads.
// Bytes are only moved, so the kernel is bandwidth-bound: 3 bytes read and 3 written per pixel.
//
// orient_rgb_kernel   grid (ceil(W'max / 64), ceil(H'max / 64), N), 256 threads; the frame's table entry is a kernel
//                     argument read with a uniform index.  A workgroup owns one 64 x 64 tile of OUTPUT pixels (output
//                     groups of 4 pixels then start at multiples of 4 in x', so that a row whose first byte is 4-byte
//                     aligned leaves as whole dwords); a thread owns 4 of the tile's 1024 groups of 4 consecutive pixels,
//                     group g = tid + 256 k: tile row g >> 4, pixels 4 (g & 15) .. + 3 -- the 16 lanes of a row segment
//                     touch 192 consecutive bytes, a wave four rows.
//   o = 1..4          rows stay rows, no LDS: the thread reads the matching source group (for o = 2, 3 the mirrored one,
//                     whose pixel order it reverses in registers) and writes its own.
//   o = 5..8          rows become columns.  The tile's source pixels -- 64 x 64 too, the same tile seen from the other
//                     side -- are read as row segments exactly as above, unpacked to one dword per pixel (R | G << 8 |
//                     B << 16) and kept in LDS as sm[y][x], dword pitch 65: 16640 bytes, which leaves the 8 workgroups
//                     per CU that the wave limit allows.  After one barrier the thread of an output group reads its 4
//                     pixels down a source column and packs them.
//                     Neither global side does strided traffic: both are the row segments of o = 1..4.
//   LDS banks         Model (the one tests/test_lds_bank_model.py uses for this part): 64 banks of 4 bytes, bank = dword
//                     address mod 64; the lanes of a wave conflict when they touch DIFFERENT dwords of one bank.  Both
//                     accesses below are one dword per lane and hit 64 different banks with the 64 lanes of a wave, so
//                     they are conflict-free however the hardware groups the lanes of a ds_read_b32 / ds_write_b32:
//                       write i (0..3) of a load group: dword 65 y + 4 l + i, l = lane & 15, y = y0 + (lane >> 4):
//                         bank = (y + 4 l + i) mod 64; 4 l is a multiple of 4 and y - y0 covers 0..3: 64 values.
//                       read i of a store group: pixel (y, x) = (+-(4 l + i) + c1, +-r + c2), r = r0 + (lane >> 4):
//                         bank = (65 y + x) mod 64 = (+-(4 l + i) +- r + c) mod 64: again 16 multiples of 4 plus 4
//                         consecutive values, 64 banks.  With pitch 64 the same read would put the 16 lanes of a row on
//                         ONE bank (a 16-way conflict); one dword of padding per row removes it.  A ragged tile masks
//                         lanes and cannot add a conflict.
//   Either way a thread's 12 bytes of a row move as three dwords when the group is complete and its address is 4-byte
//   aligned, byte by byte otherwise (row tails, odd offsets and pitches, rows of an image whose 3 W' is no multiple of
//   4) -- into and out of the same little-endian words, so both ways give the same bytes.  Ragged tiles at the right and
//   bottom edges and 1-pixel-wide / 1-pixel-high images are the same code with bounds.  Nothing outside a declared source
//   row is read and nothing outside an output image is written.  No scratch.
// A translation unit of its own on purpose: the code of frames.hip, jpeg_dec.hip and prepost.hip is pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_orient.h"
#include "orient_exif.h"

namespace {

constexpr int kTile = 64;            // output pixels per tile side
constexpr int kPix = 4;              // pixels per group
constexpr int kThreads = 256;        // 1024 groups per tile, 4 per thread
constexpr int kLdsPitch = kTile + 1; // dwords

struct Image {
  int64_t src, pitch, dst;
  int o, H, W;
};
struct ImageTable {  // a kernel argument, like frames.hip's FrameTable
  Image f[CODETR_PREPROCESS_BATCH_MAX];
};

typedef unsigned u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// npx (1..4) pixels at p -> one dword per pixel; reads exactly 3 npx bytes
__device__ __forceinline__ void load_group(const unsigned char* __restrict__ p, int npx, unsigned (&px)[kPix]) {
  unsigned w[3] = {0, 0, 0};
  if (npx == kPix && aligned4(p)) {
    const u32x3_a4 v = *reinterpret_cast<const u32x3_a4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z;
  } else {
#pragma unroll
    for (int k = 0; k < 3 * kPix; ++k)
      if (k < 3 * npx) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
  }
  px[0] = w[0] & 0xFFFFFFu;
  px[1] = (w[0] >> 24 | w[1] << 8) & 0xFFFFFFu;
  px[2] = (w[1] >> 16 | w[2] << 16) & 0xFFFFFFu;
  px[3] = w[2] >> 8;
}

// npx (1..4) pixels, one dword each (the top byte zero) -> 3 npx bytes at q
__device__ __forceinline__ void store_group(unsigned char* __restrict__ q, int npx, const unsigned (&px)[kPix]) {
  if (npx == kPix && aligned4(q)) {
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

// grid (ceil(W'max / 64), ceil(H'max / 64), N)
__global__ __launch_bounds__(kThreads) void orient_rgb_kernel(const unsigned char* __restrict__ src, ImageTable tab,
                                                              unsigned char* __restrict__ dst) {
  __shared__ unsigned sm[kTile * kLdsPitch];
  const Image& im = tab.f[blockIdx.z];  // (uniform: the entry comes through the scalar cache)
  const int o = im.o, H = im.H, W = im.W;
  const bool turned = o >= 5;
  const int Ho = turned ? W : H, Wo = turned ? H : W;  // the output image
  const int ty = blockIdx.y * kTile, tx = blockIdx.x * kTile;
  if (ty >= Ho || tx >= Wo) return;  // (uniform)
  const int nr = min(kTile, Ho - ty), nc = min(kTile, Wo - tx);  // output rows and columns of this tile
  const unsigned char* __restrict__ s = src + im.src;
  unsigned char* __restrict__ d = dst + im.dst;
  const int row0 = threadIdx.x >> 4, col = (threadIdx.x & 15) * kPix;

  if (!turned) {
    const bool flip_x = o == 2 || o == 3, flip_y = o == 3 || o == 4;
#pragma unroll
    for (int k = 0; k < kTile / 16; ++k) {
      const int r = row0 + 16 * k;
      if (r >= nr || col >= nc) continue;
      const int npx = min(kPix, nc - col);
      const int yo = ty + r, xo = tx + col;
      const int ys = flip_y ? H - 1 - yo : yo;
      const int xs = flip_x ? W - xo - npx : xo;  // the source group: mirrored, it ends where the output group starts
      unsigned px[kPix];
      load_group(s + (int64_t)ys * im.pitch + (int64_t)xs * 3, npx, px);
      if (flip_x) {  // source pixel npx - 1 - i is output pixel i
        unsigned t[kPix];
#pragma unroll
        for (int i = 0; i < kPix; ++i) t[i] = px[i];
        if (npx == 4) {
          px[0] = t[3], px[1] = t[2], px[2] = t[1], px[3] = t[0];
        } else if (npx == 3) {
          px[0] = t[2], px[1] = t[1], px[2] = t[0];
        } else if (npx == 2) {
          px[0] = t[1], px[1] = t[0];
        }
      }
      store_group(d + ((int64_t)yo * Wo + xo) * 3, npx, px);
    }
    return;
  }

  // o = 5..8: output (y', x') is source (y, x) with x = y' or W-1-y', y = x' or H-1-x'.  The tile's source pixels are the
  // nr columns from x_lo and the nc rows from y_lo; sm[ly][lx] is source pixel (y_lo + ly, x_lo + lx).
  const bool flip_r = o == 7 || o == 8;  // y' = W-1-x
  const bool flip_c = o == 6 || o == 7;  // x' = H-1-y
  const int x_lo = flip_r ? W - ty - nr : ty, y_lo = flip_c ? H - tx - nc : tx;
#pragma unroll
  for (int k = 0; k < kTile / 16; ++k) {
    const int ly = row0 + 16 * k;
    if (ly >= nc || col >= nr) continue;
    const int npx = min(kPix, nr - col);
    unsigned px[kPix];
    load_group(s + (int64_t)(y_lo + ly) * im.pitch + (int64_t)(x_lo + col) * 3, npx, px);
#pragma unroll
    for (int i = 0; i < kPix; ++i) sm[ly * kLdsPitch + col + i] = px[i];  // (col + 3 < 64: inside the row; beyond npx unread)
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTile / 16; ++k) {
    const int r = row0 + 16 * k;
    if (r >= nr || col >= nc) continue;
    const int npx = min(kPix, nc - col);
    const int lx = flip_r ? nr - 1 - r : r;
    unsigned px[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const int c = min(col + i, nc - 1);  // (a lane beyond the tile's columns reads a pixel it will not store)
      px[i] = sm[(flip_c ? nc - 1 - c : c) * kLdsPitch + lx];
    }
    store_group(d + ((int64_t)(ty + r) * Wo + tx + col) * 3, npx, px);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// rows of `rb` bytes, `rows` of them `pitch` apart from `off`: all inside [0, total)
bool rows_inside(int64_t off, int64_t pitch, int64_t rb, int64_t rows, int64_t total) {
  if (off > total || rb > total - off) return false;
  return rows == 1 || pitch <= (total - off - rb) / (rows - 1);
}

}  // namespace

extern "C" int codetr_orient_abi_version(void) { return CODETR_ORIENT_ABI_VERSION; }

extern "C" int codetr_orient_exif(const unsigned char* file_host, int64_t bytes) {
  if (!file_host || bytes <= 0) return CODETR_E_BADARG;
  return orient::exif_orientation(file_host, bytes);
}

extern "C" int codetr_orient_rgb_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host,
                                    void* dst_dev, int64_t dst_bytes) {
  if (!src_dev || !rows_host || !dst_dev || src_bytes <= 0 || dst_bytes <= 0 || N <= 0) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  {  // src and dst are different buffers
    const uintptr_t a = (uintptr_t)src_dev, b = (uintptr_t)dst_dev;
    if (a < b + (uintptr_t)dst_bytes && b < a + (uintptr_t)src_bytes) return CODETR_E_BADARG;
  }
  ImageTable tab = {};
  int64_t Hmax = 0, Wmax = 0;  // of the output images
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = rows_host + CODETR_ORIENT_ROW_INTS * n;
    const int64_t o = r[0], H = r[1], W = r[2], off = r[3], pitch = r[4], dst = r[5];
    if (o < 1 || o > 8 || H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (off < 0 || pitch < 3 * W || !rows_inside(off, pitch, 3 * W, H, src_bytes)) return CODETR_E_BADARG;
    if (dst < 0 || dst > dst_bytes || H * W * 3 > dst_bytes - dst) return CODETR_E_BADARG;
    for (int64_t m = 0; m < n; ++m) {  // two output images may not share a byte
      const int64_t o2 = tab.f[m].dst, e2 = o2 + (int64_t)tab.f[m].H * tab.f[m].W * 3;
      if (dst < e2 && o2 < dst + H * W * 3) return CODETR_E_BADARG;
    }
    tab.f[n] = Image{off, pitch, dst, (int)o, (int)H, (int)W};
    const int64_t Ho = o >= 5 ? W : H, Wo = o >= 5 ? H : W;
    Hmax = Ho > Hmax ? Ho : Hmax;
    Wmax = Wo > Wmax ? Wo : Wmax;
  }
  const dim3 grid((unsigned)((Wmax + kTile - 1) / kTile), (unsigned)((Hmax + kTile - 1) / kTile), (unsigned)N);
  hipLaunchKernelGGL(orient_rgb_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned char*>(src_dev), tab, static_cast<unsigned char*>(dst_dev));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}
