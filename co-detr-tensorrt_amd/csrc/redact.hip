// The redaction of include/codetr_redact.h: codetr_redact_detections_*, in place in the packed RGB images.
//
// redact_kernel  one 256-thread workgroup per 64 x 64-pixel tile of one image: a multiple of every allowed cell, so a
//                workgroup owns whole cells and FILL and PIXELATE are safe in place in one launch.  A thread owns the
//                column x = lane of the 16 tile rows of its wave.
//   Gather   the workgroup walks the image's detection rows 256 at a time.  A thread evaluates one row (selection and
//            region, the header's rule) and appends the region to an LDS list when it reaches the tile; then every thread
//            ORs the listed regions into the 16-bit mask of its own pixels.  A round per 256 rows, so 4096 rows that all
//            reach one tile are all honoured; the mask is a union, so the order inside a round does not matter.
//   Exit     a tile that nothing reaches returns before it touches a pixel.
//   Pixels   the tile's rows are read as the ALIGNED dwords that cover each row segment (a wave per row, a lane per dword;
//            image offsets and row pitches carry no alignment, so the two end dwords of a segment are assembled from
//            their bytes inside the segment), kept in LDS in that layout, changed there, and stored the same way: a dword
//            whose four bytes all changed goes out whole, any other byte by byte -- an unmasked pixel is never written.
//   Phases   kInPlace  FILL, PIXELATE: mask, (PIXELATE: tile -> cell sums -> means), new bytes, store.
//            kMeans    BLUR, first launch: the regions grown by one cell; a reached tile writes the means of its cells to
//                      the workspace.  It writes no pixel.
//            kApply    BLUR, second launch: mask, the (64 / cell + 2)^2 means around the tile from the workspace (indices
//                      clamped to the grid; the first launch wrote every one a masked pixel uses), the tent, store.  It
//                      reads no pixel, so no workgroup reads what another may have written.
// fp32 with one rounding per operation: contraction is off for the whole file.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_redact.h"
#include "box_prims.h"
#include "redact_args.h"

namespace {

using redact_args::Image;
using redact_args::Table;

constexpr int kTile = CODETR_REDACT_TILE, kThreads = 256, kRowsPerThread = 16;
constexpr int kRowDwords = (3 + 3 * kTile + 3) / 4;  // 49: a 192-byte segment at any byte phase
constexpr int kMaxCells = (kTile / 4) * (kTile / 4), kMaxStage = (kTile / 4 + 2) * (kTile / 4 + 2);
enum { kInPlace = 0, kMeans = 1, kApply = 2 };
static_assert(kTile == 64 && kThreads == 4 * kTile && kRowsPerThread * 4 == kTile, "a lane per column, 16 rows per wave");
static_assert(kRowDwords <= 64, "a lane per dword of a row segment");

struct Params {
  int mode, shape, cell, lc;  // lc = log2(cell)
  float score_thr, expand;
  int fill[3];
  int C;
};

__device__ __forceinline__ float clamp_coord(float v) { return fminf(fmaxf(v, -16384.f), 16383.f); }

// the region of a redacted row; false when it does not exist
__device__ __forceinline__ bool region_of(float x1, float y1, float x2, float y2, float expand, int4* r) {
  x1 = clamp_coord(x1), y1 = clamp_coord(y1), x2 = clamp_coord(x2), y2 = clamp_coord(y2);
  const float w = x2 - x1, h = y2 - y1;
  const float ex = expand * w, ey = expand * h;
  const float a1 = clamp_coord(x1 - ex), a2 = clamp_coord(x2 + ex);
  const float b1 = clamp_coord(y1 - ey), b2 = clamp_coord(y2 + ey);
  *r = make_int4((int)floorf(a1), (int)floorf(b1), (int)ceilf(a2) - 1, (int)ceilf(b2) - 1);
  return r->z >= r->x && r->w >= r->y;
}

// the first byte of the tile's row `y` of an image and the segment's byte phase inside its first aligned dword
__device__ __forceinline__ unsigned char* row_segment(unsigned char* img, int y, int W, int tx0, int* phase) {
  unsigned char* seg = img + ((int64_t)y * W + tx0) * 3;
  *phase = (int)((uintptr_t)seg & 3u);
  return seg;
}

// grid (ceil(Wmax / 64), ceil(Hmax / 64), N)
template <class T, int kPhase>
__global__ __launch_bounds__(kThreads) void redact_kernel(unsigned char* __restrict__ buf, Table tab,
                                                          const T* __restrict__ boxes, const T* __restrict__ scores,
                                                          const int64_t* __restrict__ labels,
                                                          const int* __restrict__ count, int Q,
                                                          const unsigned char* __restrict__ select, Params p,
                                                          unsigned* __restrict__ work) {
  __shared__ int4 s_reg[kThreads];
  __shared__ int s_n;
  __shared__ unsigned s_row[kTile][kRowDwords];
  __shared__ unsigned long long s_mask[kTile];
  __shared__ int s_sum[kMaxCells * 3];
  __shared__ unsigned s_mean[kMaxStage];

  const int n = blockIdx.z;
  const Image im = tab.img[n];
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  if (tx0 >= im.W || ty0 >= im.H) return;  // a tile beyond its image (uniform)
  const int tx1 = min(tx0 + kTile, im.W) - 1, ty1 = min(ty0 + kTile, im.H) - 1;
  const int tw = tx1 - tx0 + 1, th = ty1 - ty0 + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = tx0 + lane, y0 = ty0 + wave * kRowsPerThread;
  const T* ibox = boxes + (size_t)n * Q * 4;
  const T* iscore = scores + (size_t)n * Q;
  const int64_t* ilabel = labels + (size_t)n * Q;
  const int cnt = min(max(count[n], 0), Q);
  const int c = p.cell, lc = p.lc;
  const int grow = kPhase == kMeans ? c : 0;

  // ---- gather: the regions that reach this tile, a round per 256 rows
  unsigned mask = 0;  // bit r: the pixel (x, y0 + r) is masked
  int hits = 0;       // (uniform)
  for (int base = 0; base < cnt; base += kThreads) {
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int j = base + tid;
    if (j < cnt) {
      const float s = to_f32(iscore[j]);
      const int64_t label = ilabel[j];
      const float x1 = to_f32(ibox[4 * j]), y1 = to_f32(ibox[4 * j + 1]);
      const float x2 = to_f32(ibox[4 * j + 2]), y2 = to_f32(ibox[4 * j + 3]);
      const bool chosen = select == nullptr || (label >= 0 && label < p.C && select[label] != 0);
      int4 r;
      if (s > p.score_thr && chosen && __builtin_isfinite(x1) && __builtin_isfinite(y1) && __builtin_isfinite(x2) &&
          __builtin_isfinite(y2) && region_of(x1, y1, x2, y2, p.expand, &r)) {
        const bool in_image = r.x <= im.W - 1 && r.z >= 0 && r.y <= im.H - 1 && r.w >= 0;
        if (in_image && r.x - grow <= tx1 && r.z + grow >= tx0 && r.y - grow <= ty1 && r.w + grow >= ty0)
          s_reg[atomicAdd(&s_n, 1)] = r;
      }
    }
    __syncthreads();
    const int nr = s_n;
    hits += nr;
    if (kPhase != kMeans) {
      for (int i = 0; i < nr; ++i) {
        const int4 r = s_reg[i];
        if (x < r.x || x > r.z) continue;
        const int lo = max(r.y - y0, 0), hi = min(r.w - y0, kRowsPerThread - 1);
        if (lo > hi) continue;
        if (p.shape == CODETR_REDACT_BOX) {
          mask |= ((2u << hi) - 1u) & ~((1u << lo) - 1u);
        } else {
          const int64_t Ww = r.z - r.x + 1, Hh = r.w - r.y + 1;
          const int64_t a = (int64_t)(2 * x - r.x - r.z) * Hh, rr = Ww * Hh;
          const int64_t rest = rr * rr - a * a;
          for (int k = lo; k <= hi; ++k) {
            const int64_t b = (int64_t)(2 * (y0 + k) - r.y - r.w) * Ww;
            if (b * b <= rest) mask |= 1u << k;
          }
        }
      }
    }
    __syncthreads();  // the list is read: the next round may reset it
  }
  if (hits == 0) return;  // nothing reaches the tile: no pixel is touched

  unsigned char* img = buf + im.offset;
  const int kc = kTile >> lc;               // cells per tile side
  const int gw = (im.W + c - 1) >> lc, gh = (im.H + c - 1) >> lc;
  const int gx0 = tx0 >> lc, gy0 = ty0 >> lc;

  if (kPhase != kMeans) {  // clip the mask to the image and lay it out by tile row
    if (x > tx1) mask = 0;
    const int rows_in = ty1 - y0 + 1;  // of this thread's 16
    mask = rows_in <= 0 ? 0u : rows_in >= kRowsPerThread ? mask : mask & ((1u << rows_in) - 1u);
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
      const unsigned long long m = __ballot((mask >> r) & 1u);
      if (lane == 0) s_mask[wave * kRowsPerThread + r] = m;
    }
    if (!__syncthreads_or(mask != 0)) return;  // (an ellipse whose rectangle reaches the tile may still miss it)
  }

  const bool need_pixels = kPhase == kMeans || (kPhase == kInPlace && p.mode == CODETR_REDACT_PIXELATE);
  if (need_pixels) {
    // ---- the tile into LDS: a wave per row, a lane per aligned dword
    for (int i = tid; i < kc * kc * 3; i += kThreads) s_sum[i] = 0;
    for (int r = wave; r < th; r += 4) {
      int phase;
      const unsigned char* seg = row_segment(img, ty0 + r, im.W, tx0, &phase);
      const int len = 3 * tw, ndw = (phase + len + 3) >> 2;
      if (lane < ndw) {
        const int k0 = 4 * lane - phase;  // the segment byte of the dword's first byte
        unsigned v = 0;
        if (k0 >= 0 && k0 + 4 <= len) {
          v = *reinterpret_cast<const unsigned*>(seg + k0);
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (k0 + b >= 0 && k0 + b < len) v |= (unsigned)seg[k0 + b] << (8 * b);
        }
        s_row[r][lane] = v;
      }
    }
    __syncthreads();
    // ---- cell sums: a thread adds its column's run inside each cell, then one LDS atomic per run and channel
    if (lane < tw) {
      int acc[3] = {0, 0, 0};
      bool any = false;
      for (int r = 0; r < kRowsPerThread; ++r) {
        const int ry = wave * kRowsPerThread + r;
        if (ry < th) {
          int phase;
          row_segment(img, ty0 + ry, im.W, tx0, &phase);
          const unsigned char* px = reinterpret_cast<const unsigned char*>(s_row[ry]) + phase + 3 * lane;
          acc[0] += px[0], acc[1] += px[1], acc[2] += px[2];
          any = true;
        }
        if ((((ry + 1) & (c - 1)) == 0 || r == kRowsPerThread - 1) && any) {
          int* sum = s_sum + ((ry >> lc) * kc + (lane >> lc)) * 3;
          atomicAdd(sum, acc[0]), atomicAdd(sum + 1, acc[1]), atomicAdd(sum + 2, acc[2]);
          acc[0] = acc[1] = acc[2] = 0;
          any = false;
        }
      }
    }
    __syncthreads();
    if (tid < kc * kc) {
      const int cx = tid & (kc - 1), cy = tid >> (6 - lc);
      const int cw = min(c, tw - cx * c), ch = min(c, th - cy * c);
      if (cw > 0 && ch > 0) {
        const int np = cw * ch;
        const unsigned m0 = (unsigned)((s_sum[3 * tid] + np / 2) / np), m1 = (unsigned)((s_sum[3 * tid + 1] + np / 2) / np);
        const unsigned m2 = (unsigned)((s_sum[3 * tid + 2] + np / 2) / np);
        const unsigned packed = m0 | (m1 << 8) | (m2 << 16);
        if (kPhase == kMeans) work[im.work + (int64_t)(gy0 + cy) * gw + (gx0 + cx)] = packed;  // inside the grid: cw, ch > 0
        else s_mean[tid] = packed;
      }
    }
    if (kPhase == kMeans) return;
    __syncthreads();
  }

  // ---- the new bytes of the masked pixels, into the LDS rows
  const int side = kc + 2;
  if (kPhase == kApply) {
    for (int i = tid; i < side * side; i += kThreads) {
      const int cy = min(max(gy0 - 1 + i / side, 0), gh - 1), cx = min(max(gx0 - 1 + i % side, 0), gw - 1);
      s_mean[i] = work[im.work + (int64_t)cy * gw + cx];
    }
    __syncthreads();
  }
  if (mask != 0) {
    int fx = 0, bx = 0;
    if (kPhase == kApply) {
      const int u = 2 * x + 1 - c, i0 = u >> (lc + 1);  // (an arithmetic shift: floor)
      fx = u - (i0 << (lc + 1));
      bx = i0 - (gx0 - 1);  // 0..kc
    }
#pragma unroll 4
    for (int r = 0; r < kRowsPerThread; ++r) {
      if (!((mask >> r) & 1u)) continue;
      const int ry = wave * kRowsPerThread + r;
      int v0, v1, v2;
      if (kPhase == kApply) {
        const int u = 2 * (y0 + r) + 1 - c, k0 = u >> (lc + 1);
        const int fy = u - (k0 << (lc + 1)), by = k0 - (gy0 - 1);
        const unsigned m00 = s_mean[by * side + bx], m01 = s_mean[by * side + bx + 1];
        const unsigned m10 = s_mean[(by + 1) * side + bx], m11 = s_mean[(by + 1) * side + bx + 1];
        const int wx0 = 2 * c - fx, wy0 = 2 * c - fy;
        const int w00 = wx0 * wy0, w01 = fx * wy0, w10 = wx0 * fy, w11 = fx * fy;
        const int half = 2 * c * c, sh = 2 * lc + 2;
        v0 = (w00 * (int)(m00 & 255u) + w01 * (int)(m01 & 255u) + w10 * (int)(m10 & 255u) + w11 * (int)(m11 & 255u) + half) >> sh;
        v1 = (w00 * (int)((m00 >> 8) & 255u) + w01 * (int)((m01 >> 8) & 255u) + w10 * (int)((m10 >> 8) & 255u) +
              w11 * (int)((m11 >> 8) & 255u) + half) >> sh;
        v2 = (w00 * (int)((m00 >> 16) & 255u) + w01 * (int)((m01 >> 16) & 255u) + w10 * (int)((m10 >> 16) & 255u) +
              w11 * (int)((m11 >> 16) & 255u) + half) >> sh;
      } else if (p.mode == CODETR_REDACT_PIXELATE) {
        const unsigned m = s_mean[(ry >> lc) * kc + (lane >> lc)];
        v0 = (int)(m & 255u), v1 = (int)((m >> 8) & 255u), v2 = (int)((m >> 16) & 255u);
      } else {
        v0 = p.fill[0], v1 = p.fill[1], v2 = p.fill[2];
      }
      int phase;
      row_segment(img, ty0 + ry, im.W, tx0, &phase);
      unsigned char* px = reinterpret_cast<unsigned char*>(s_row[ry]) + phase + 3 * lane;
      px[0] = (unsigned char)v0, px[1] = (unsigned char)v1, px[2] = (unsigned char)v2;
    }
  }
  __syncthreads();

  // ---- store: a wave per row with a masked pixel, a lane per aligned dword; whole where all four bytes changed
  for (int r = wave; r < th; r += 4) {
    const unsigned long long m = s_mask[r];
    if (m == 0) continue;  // (wave-uniform)
    int phase;
    unsigned char* seg = row_segment(img, ty0 + r, im.W, tx0, &phase);
    const int len = 3 * tw, ndw = (phase + len + 3) >> 2;
    if (lane < ndw) {
      const int k0 = 4 * lane - phase;
      const unsigned v = s_row[r][lane];
      bool on[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int k = k0 + b;
        on[b] = k >= 0 && k < len && ((m >> (k / 3)) & 1ull);
      }
      if (on[0] && on[1] && on[2] && on[3]) {
        *reinterpret_cast<unsigned*>(seg + k0) = v;
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (on[b]) seg[k0 + b] = (unsigned char)(v >> (8 * b));
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

template <class T, int kPhase>
void launch_phase(hipStream_t stream, dim3 grid, void* buf, const Table& tab, const void* boxes, const void* scores,
                  const int64_t* labels, const int* count, int64_t Q, const unsigned char* select, const Params& p,
                  void* work) {
  hipLaunchKernelGGL((redact_kernel<T, kPhase>), grid, dim3(kThreads), 0, stream, static_cast<unsigned char*>(buf), tab,
                     static_cast<const T*>(boxes), static_cast<const T*>(scores), labels, count, (int)Q, select, p,
                     static_cast<unsigned*>(work));
}

template <class T>
int launch_redact(void* stream, void* buf, int64_t buf_bytes, int64_t N, const int64_t* images, const void* boxes,
                  const void* scores, const int64_t* labels, const int* count, int64_t Q, const unsigned char* select,
                  int64_t C, int mode, int shape, int cell, float score_thr, float expand, uint32_t fill_rgb, void* work,
                  int64_t work_bytes) {
  Table tab = {};
  int64_t Hmax = 0, Wmax = 0;
  const int rc = redact_args::check(buf, buf_bytes, N, images, boxes, scores, labels, count, Q, select, C, mode, shape, cell,
                                    score_thr, expand, fill_rgb, work, work_bytes, &tab, &Hmax, &Wmax);
  if (rc != 0) return rc;
  Params p;
  p.mode = mode, p.shape = shape, p.cell = cell, p.lc = redact_args::log2_cell(cell);
  p.score_thr = score_thr, p.expand = expand;
  p.fill[0] = (int)((fill_rgb >> 16) & 255u), p.fill[1] = (int)((fill_rgb >> 8) & 255u), p.fill[2] = (int)(fill_rgb & 255u);
  p.C = select ? (int)C : 0;
  const dim3 grid((unsigned)((Wmax + kTile - 1) / kTile), (unsigned)((Hmax + kTile - 1) / kTile), (unsigned)N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == CODETR_REDACT_BLUR) {
    launch_phase<T, kMeans>(st, grid, buf, tab, boxes, scores, labels, count, Q, select, p, work);
    launch_phase<T, kApply>(st, grid, buf, tab, boxes, scores, labels, count, Q, select, p, work);
  } else {
    launch_phase<T, kInPlace>(st, grid, buf, tab, boxes, scores, labels, count, Q, select, p, nullptr);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

extern "C" {

int codetr_redact_abi_version(void) { return CODETR_REDACT_ABI_VERSION; }

int64_t codetr_redact_work_bytes(int64_t N, const int64_t* images_host, int64_t cell) {
  const int64_t cells = redact_args::count_cells(N, images_host, cell, nullptr);
  return cells < 0 ? cells : 4 * cells;
}

#define CODETR_REDACT_ENTRY(SUFFIX, TYPE)                                                                                  \
  int codetr_redact_detections_##SUFFIX(void* stream, void* buf_dev, int64_t buf_bytes, int64_t N,                        \
                                        const int64_t* images_host, const void* boxes_dev, const void* scores_dev,        \
                                        const int64_t* labels_dev, const int* count_dev, int64_t Q,                       \
                                        const unsigned char* select_dev, int64_t C, int mode, int shape, int cell,        \
                                        float score_thr, float expand, uint32_t fill_rgb, void* work_dev,                  \
                                        int64_t work_bytes) {                                                              \
    return launch_redact<TYPE>(stream, buf_dev, buf_bytes, N, images_host, boxes_dev, scores_dev, labels_dev, count_dev,  \
                               Q, select_dev, C, mode, shape, cell, score_thr, expand, fill_rgb, work_dev, work_bytes);   \
  }
CODETR_REDACT_ENTRY(f16, _Float16)
CODETR_REDACT_ENTRY(bf16, Bf16)
CODETR_REDACT_ENTRY(f32, float)
#undef CODETR_REDACT_ENTRY

}  // extern "C"
