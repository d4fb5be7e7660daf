// Camera-motion estimate for the tracker: codetr_motion_estimate_u8 of include/codetr_motion.h, which states the rule
// operation by operation (integers, one fp32 division per axis at the end); this file follows that text.  Three launches
// on the caller's stream, nothing host-visible in between; the thumbnails and the votes live in the caller's scratch.
// codetr_motion_estimate2_u8 (the header's version 2, the similarity model) adds two launches behind them: see the section
// at the end of the kernels.
//
// motion_thumb_kernel     grid (bands, th, N), 256 threads: one workgroup per band of <= 1024 source pixels (a whole number
//                        of cells) of one thumbnail row.  A byte mover over 3-byte pixels: the k source rows of the band come
//                        in four at a time as whole aligned dwords, consecutive threads consecutive dwords, into LDS (a
//                        dword that is not wholly inside the image is put together from its bytes inside: nothing outside
//                        an image is read); then one thread per pixel reads its three bytes from LDS and adds the gray to
//                        its cell (integer LDS atomics: the order does not matter).  LDS 13 KB.
// motion_match_kernel     grid (blocks, N), 256 threads: one workgroup per 16 x 16 block of a row.  The block of the previous
//                        thumbnail (256 bytes) and its (16 + 2 R)^2 search region of the current one (rows at a pitch of 48
//                        bytes) sit in LDS, 2.6 KB + the (2 R + 1)^2 sums.  A thread owns a displacement: per block row it
//                        reads the previous row as four broadcast dwords and the current row as five aligned dwords, shifts
//                        them into place and takes four v_sad_u8 (4 bytes each); lanes of a wave hold neighbouring dx, so
//                        their dwords coincide or are neighbours (no bank conflict beyond the 12-dword row step).  The best
//                        displacement is one 64-bit minimum (sum, distance, dy, dx packed) by wave shuffles.
//                        Workgroup 0 of a row also records whether the row has a usable predecessor: the third launch never
//                        reads a state.
// motion_finish_kernel    grid N, 128 threads (a thread per block): medians by rank, agreement, the two divisions; the
//                        workgroup of a stream's last row then replaces the stream's state -- in a launch of its own because
//                        the second launch reads the states (a stream's first row) that this one overwrites.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_motion.h"

namespace {

constexpr int kThumbSide = CODETR_MOTION_GRID_MAX;
constexpr int kThumbBytes = kThumbSide * kThumbSide;      // 25600: one thumbnail of the scratch and of a state
constexpr int kStateBytes = 16 + kThumbBytes;
constexpr int kVoteInts = 4 + 3 * CODETR_MOTION_MAX_BLOCKS;  // per row: {usable predecessor, 0, 0, 0}, then {textured, vx, vy}
constexpr int kThreads = 256;
constexpr int kBandPixels = 1024;
constexpr int kBandRows = 4;                               // source rows staged per barrier
constexpr int kBandWords = (3 + 3 * kBandPixels + 3) / 4 + 3;  // 772: a band row from its aligned dword down
constexpr int kPitch = CODETR_MOTION_BLOCK + 2 * CODETR_MOTION_SEARCH_MAX;  // 48
constexpr int kMaxDisp = (2 * CODETR_MOTION_SEARCH_MAX + 1) * (2 * CODETR_MOTION_SEARCH_MAX + 1);
constexpr int kFinishThreads = 128;
static_assert(CODETR_MOTION_BLOCK == 16 && kPitch % 4 == 0, "the match kernel's row arithmetic");
static_assert(CODETR_MOTION_MAX_BLOCKS <= kFinishThreads, "a thread per block");
static_assert((kThumbSide - 2) / 16 * ((kThumbSide - 2) / 16) <= CODETR_MOTION_MAX_BLOCKS, "every block has a vote slot");

struct Row {
  int64_t off;
  int H, W, k, th, tw, nbx, nby;
  int stream, prev, same, last;  // prev: the row before it of its stream (-1: the state); same: that row has its H and W
};
struct RowTab {  // a kernel argument, like prepost.hip's BatchTable
  Row r[CODETR_PREPROCESS_BATCH_MAX];
};

__device__ __forceinline__ int absdiff(int a, int b) { return a > b ? a - b : b - a; }

// ---- 1. thumbnails -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void motion_thumb_kernel(const unsigned char* __restrict__ src, RowTab tab,
                                                                unsigned char* __restrict__ thumbs) {
  __shared__ unsigned stage[kBandRows][kBandWords];
  __shared__ int acc[kThumbSide];
  const Row& r = tab.r[blockIdx.z];  // (uniform)
  const int ty = blockIdx.y, tid = threadIdx.x, k = r.k;
  const int cells = max(1, kBandPixels / k);
  const int c0 = blockIdx.x * cells;
  if (ty >= r.th || c0 >= r.tw) return;
  const int nc = min(cells, r.tw - c0), npx = nc * k;  // npx <= 1024 (k <= 1024)
  for (int c = tid; c < nc; c += kThreads) acc[c] = 0;
  const unsigned char* img = src + r.off;
  const unsigned char* img_end = img + (int64_t)r.H * r.W * 3;

  for (int y0 = 0; y0 < k; y0 += kBandRows) {  // (uniform)
    const int nr = min(kBandRows, k - y0);
#pragma unroll
    for (int rr = 0; rr < kBandRows; ++rr) {
      if (rr >= nr) break;
      const unsigned char* p = img + ((int64_t)(ty * k + y0 + rr) * r.W + (int64_t)c0 * k) * 3;
      const int lead = (int)((uintptr_t)p & 3u);
      const unsigned char* a = p - lead;
      const int ndw = (lead + npx * 3 + 3) >> 2;  // <= 769
      for (int i = tid; i < ndw; i += kThreads) {
        const unsigned char* q = a + 4 * i;
        unsigned w = 0;
        if (q >= img && q + 4 <= img_end) {
          w = *reinterpret_cast<const unsigned*>(q);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (q + e >= img && q + e < img_end) w |= (unsigned)q[e] << (8 * e);
        }
        stage[rr][i] = w;
      }
    }
    __syncthreads();
    for (int px = tid; px < npx; px += kThreads) {
      const int cell = px / k;
      int sum = 0;
#pragma unroll
      for (int rr = 0; rr < kBandRows; ++rr) {
        if (rr >= nr) break;
        const unsigned char* p = img + ((int64_t)(ty * k + y0 + rr) * r.W + (int64_t)c0 * k) * 3;
        const unsigned char* b = reinterpret_cast<const unsigned char*>(stage[rr]) + ((uintptr_t)p & 3u) + 3 * px;
        sum += (77 * b[0] + 150 * b[1] + 29 * b[2] + 128) >> 8;
      }
      atomicAdd(&acc[cell], sum);
    }
    __syncthreads();
  }
  const int kk = k * k;
  for (int c = tid; c < nc; c += kThreads)
    thumbs[(int64_t)blockIdx.z * kThumbBytes + ty * r.tw + c0 + c] = (unsigned char)((acc[c] + kk / 2) / kk);
}

// ---- 2. the votes of the blocks ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void motion_match_kernel(RowTab tab, int R, int texture,
                                                                const unsigned char* __restrict__ states,
                                                                const unsigned char* __restrict__ thumbs,
                                                                int* __restrict__ votes) {
  __shared__ unsigned Pw[64];                    // the block of the previous thumbnail, 16 rows of 4 dwords
  __shared__ unsigned Cw[kPitch * kPitch / 4 + 4];  // its search region of the current one, rows of 12 dwords
  __shared__ int S[kMaxDisp];
  __shared__ int red[kThreads / 64];
  __shared__ unsigned long long red_key[kThreads / 64];
  const int n = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Row& r = tab.r[n];  // (uniform)
  const unsigned char* P;
  bool ok;
  if (r.prev >= 0) {
    ok = r.same != 0;
    P = thumbs + (int64_t)r.prev * kThumbBytes;
  } else {
    const unsigned char* st = states + (int64_t)r.stream * kStateBytes;
    const int* h = reinterpret_cast<const int*>(st);
    ok = h[0] != 0 && h[1] == r.H && h[2] == r.W && h[3] == r.k;
    P = st + 16;
  }
  int* vote = votes + (int64_t)n * kVoteInts;
  if (b == 0 && tid == 0) vote[0] = ok ? 1 : 0;
  if (!ok || b >= r.nbx * r.nby) return;  // (uniform)
  const unsigned char* C = thumbs + (int64_t)n * kThumbBytes;
  const int by = b / r.nbx, bx = b - by * r.nbx, tw = r.tw, side = 16 + 2 * R;
  unsigned char* Pb = reinterpret_cast<unsigned char*>(Pw);
  unsigned char* Cb = reinterpret_cast<unsigned char*>(Cw);
  Pb[tid] = P[(R + 16 * by + (tid >> 4)) * tw + R + 16 * bx + (tid & 15)];
  for (int i = tid; i < side * side; i += kThreads) {  // rows 16 by .. 16 by + side - 1 <= th - 1, columns likewise
    const int y = i / side, x = i - y * side;
    Cb[y * kPitch + x] = C[(16 * by + y) * tw + 16 * bx + x];
  }
  if (tid < 4) Cw[kPitch * kPitch / 4 + tid] = 0;  // (read as the dword behind the last row, shifted out)
  __syncthreads();

  {  // textured?
    const int y = tid >> 4, x = tid & 15, v = Pb[tid];
    int t = (x < 15 ? absdiff(v, Pb[tid + 1]) : 0) + (y < 15 ? absdiff(v, Pb[tid + 16]) : 0);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) t += __shfl_xor(t, m, 64);
    if (lane == 0) red[wave] = t;
    __syncthreads();
    t = red[0] + red[1] + red[2] + red[3];
    if (t < texture * 256) {  // (uniform)
      if (tid < 3) vote[4 + 3 * b + tid] = 0;
      return;
    }
  }

  const int w = 2 * R + 1, nd = w * w;
  unsigned long long best = ~0ull;
  for (int d = tid; d < nd; d += kThreads) {
    const int dyi = d / w, dxi = d - dyi * w;  // (dy, dx) = (dyi - R, dxi - R): the region's row dyi, column dxi
    const int sh = (dxi & 3) * 8;
    unsigned sad = 0;
#pragma unroll 4
    for (int y = 0; y < 16; ++y) {
      const unsigned* c = Cw + (dyi + y) * (kPitch / 4) + (dxi >> 2);
      const unsigned c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4];
      const unsigned* p = Pw + 4 * y;
      sad = __builtin_amdgcn_sad_u8(p[0], (unsigned)((((unsigned long long)c1 << 32) | c0) >> sh), sad);
      sad = __builtin_amdgcn_sad_u8(p[1], (unsigned)((((unsigned long long)c2 << 32) | c1) >> sh), sad);
      sad = __builtin_amdgcn_sad_u8(p[2], (unsigned)((((unsigned long long)c3 << 32) | c2) >> sh), sad);
      sad = __builtin_amdgcn_sad_u8(p[3], (unsigned)((((unsigned long long)c4 << 32) | c3) >> sh), sad);
    }
    S[d] = (int)sad;
    const int dy = dyi - R, dx = dxi - R;
    const unsigned long long key = ((unsigned long long)sad << 32) | ((unsigned)(dy * dy + dx * dx) << 12) |
                                   ((unsigned)dyi << 6) | (unsigned)dxi;
    best = key < best ? key : best;
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)best, m, 64), hi = __shfl_xor((unsigned)(best >> 32), m, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    best = o < best ? o : best;
  }
  if (lane == 0) red_key[wave] = best;
  __syncthreads();  // (S is complete as well)
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < kThreads / 64; ++i) best = red_key[i] < best ? red_key[i] : best;
    const int s0 = (int)(best >> 32), dyi = (int)(best >> 6) & 63, dxi = (int)best & 63;
    const auto step = [&](bool inside, int sm, int sp) -> int {
      if (!inside) return 0;
      const int den = sm - 2 * s0 + sp;
      if (den <= 0) return 0;
      const int num = 16 * (sm - sp) + den, d2 = 2 * den;
      const int q = num >= 0 ? num / d2 : -((-num + d2 - 1) / d2);  // floor
      return min(max(q, -8), 8);
    };
    const bool in_x = dxi >= 1 && dxi <= 2 * R - 1, in_y = dyi >= 1 && dyi <= 2 * R - 1;
    const int sx = step(in_x, in_x ? S[dyi * w + dxi - 1] : 0, in_x ? S[dyi * w + dxi + 1] : 0);
    const int sy = step(in_y, in_y ? S[(dyi - 1) * w + dxi] : 0, in_y ? S[(dyi + 1) * w + dxi] : 0);
    vote[4 + 3 * b] = 1;
    vote[4 + 3 * b + 1] = 16 * (dxi - R) + sx;
    vote[4 + 3 * b + 2] = 16 * (dyi - R) + sy;
  }
}

// ---- 3. the motion of every row, and the states ----------------------------------------------------------------------------
__global__ __launch_bounds__(kFinishThreads) void motion_finish_kernel(RowTab tab, int min_blocks,
                                                                      const unsigned char* __restrict__ thumbs,
                                                                      const int* __restrict__ votes,
                                                                      unsigned char* __restrict__ states,
                                                                      float* __restrict__ motion, int* __restrict__ diag) {
  __shared__ int tex[kFinishThreads], vx[kFinishThreads], vy[kFinishThreads];
  __shared__ int cnt[6];  // n, c, sum_x, sum_y, mx, my
  const int n = blockIdx.x, tid = threadIdx.x;
  const Row& r = tab.r[n];  // (uniform)
  const int* vote = votes + (int64_t)n * kVoteInts;
  const bool ok = vote[0] != 0;
  const int nb = r.nbx * r.nby;
  const bool mine = ok && tid < nb && vote[4 + 3 * tid] != 0;
  const int x = mine ? vote[4 + 3 * tid + 1] : 0, y = mine ? vote[4 + 3 * tid + 2] : 0;
  tex[tid] = mine, vx[tid] = x, vy[tid] = y;
  if (tid < 6) cnt[tid] = 0;
  __syncthreads();
  if (mine) atomicAdd(&cnt[0], 1);
  __syncthreads();
  const int nt = cnt[0];
  const bool enough = nt >= min_blocks;  // (uniform)
  if (enough) {
    if (mine) {  // the element of rank (nt - 1) / 2 in the ascending order (ties by block index) is the lower median
      int rx = 0, ry = 0;
      for (int j = 0; j < nb; ++j) {
        if (!tex[j]) continue;
        rx += vx[j] < x || (vx[j] == x && j < tid);
        ry += vy[j] < y || (vy[j] == y && j < tid);
      }
      if (rx == (nt - 1) / 2) cnt[4] = x;
      if (ry == (nt - 1) / 2) cnt[5] = y;
    }
    __syncthreads();
    if (mine && abs(x - cnt[4]) <= 16 && abs(y - cnt[5]) <= 16) {
      atomicAdd(&cnt[1], 1);
      atomicAdd(&cnt[2], x);
      atomicAdd(&cnt[3], y);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int c = cnt[1];
    const bool valid = enough && 2 * c >= nt;  // (then c >= 1: nt >= min_blocks >= 1)
    float* m = motion + 4 * (int64_t)n;
    m[0] = valid ? (float)(cnt[2] * r.k) / (float)(16 * c) : 0.f;
    m[1] = valid ? (float)(cnt[3] * r.k) / (float)(16 * c) : 0.f;
    m[2] = valid ? 1.f : 0.f;
    m[3] = 0.f;
    int* d = diag + 4 * (int64_t)n;
    d[0] = r.k, d[1] = nb, d[2] = nt, d[3] = enough ? c : 0;
  }
  if (!r.last) return;  // (uniform)
  unsigned* st = reinterpret_cast<unsigned*>(states + (int64_t)r.stream * kStateBytes);
  if (tid == 0) st[0] = 1u, st[1] = (unsigned)r.H, st[2] = (unsigned)r.W, st[3] = (unsigned)r.k;
  const unsigned* t = reinterpret_cast<const unsigned*>(thumbs + (int64_t)n * kThumbBytes);
  const int bytes = r.th * r.tw;
  for (int i = tid; i < kThumbBytes / 4; i += kFinishThreads) {  // the thumbnail, zero behind its th * tw bytes
    const int left = bytes - 4 * i;
    st[4 + i] = left >= 4 ? t[i] : (left <= 0 ? 0u : t[i] & ((1u << (8 * left)) - 1u));
  }
}

// ---- the similarity model (version 2 of the header) ---------------------------------------------------------------------
// Two launches behind the three above, which run as they are (the third writes its translation row into the scratch):
// motion_sim_pairs_kernel grid (kSimGroups, N), 256 threads: the row's textured blocks, numbered in ascending block order,
//                        sit in LDS as one int4 each (block indices and 256 g + v: a ds_read_b128 that every lane of a
//                        wave reads at one address); lanes over the n * n ordered index pairs, a row's share strided over its
//                        kSimGroups workgroups; a lane with an eligible pair counts the pair's inliers over all blocks with
//                        the reduced int32 test of the header.  Best pair of the workgroup: one 64-bit maximum (count, ~i,
//                        ~j) by wave shuffles, then over the waves in LDS; one slot per workgroup in the scratch.
// motion_sim_fit_kernel   grid N, 128 threads (a thread per textured block): the maximum of the row's slots, the inliers of
//                        that pair, the refit's int64 sums by LDS atomics (integers: the order does not matter), the four
//                        divisions; or the translation row, or zeros.
constexpr int kSimGroups = 8;
constexpr int kSimThreads = 256;
constexpr int kSimSlotInts = 4;  // per (row, workgroup): key high, key low, eligible pairs, 0
constexpr int kSimRowInts = 8 + kSimGroups * kSimSlotInts;  // per row; the scratch holds the translation rule's motion
                                                           // [N, 4], then its diag [N, 4], then the slots [N, kSimGroups]
static_assert(CODETR_MOTION_MAX_BLOCKS <= 128, "the compaction below ranks over the first two waves' lanes");

// The textured blocks of a row in ascending block order -> pts[t] = {bx, by, 256 bx + vx, 256 by + vy}; returns n.  Every
// thread of the workgroup calls it (blockDim.x a multiple of 64, >= 128); two barriers.
__device__ __forceinline__ int sim_gather(const Row& r, const int* __restrict__ vote, int4* pts, int* wcount) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = vote[0] != 0 ? r.nbx * r.nby : 0;  // (uniform)
  const bool mine = tid < nb && vote[4 + 3 * tid] != 0;
  const unsigned long long b = __ballot(mine);
  if (lane == 0 && wave < 2) wcount[wave] = __popcll(b);
  __syncthreads();
  if (mine) {
    const int t = (wave ? wcount[0] : 0) + __popcll(b & ((1ull << lane) - 1ull));
    const int by = tid / r.nbx, bx = tid - by * r.nbx;
    pts[t] = make_int4(bx, by, 256 * bx + vote[4 + 3 * tid + 1], 256 * by + vote[4 + 3 * tid + 2]);
  }
  __syncthreads();
  return wcount[0] + wcount[1];
}

// the pair (i, j) of the header in reduced form: r' = F(m) - F(i), F(m) = A' G_m + B' G_m_perp - dd' W_m, against 16 dd'.
// Every factor is below 2^17 in magnitude and every product below 2^21 (the header's bound), so the products are exact as
// 24-bit multiplies (v_mul_i32_i24, full rate; v_mul_lo_u32 is quarter rate); the test is branch-free so that the loop over
// the blocks keeps several LDS reads in flight.
struct SimPair {
  int A, B, dd, fx, fy, tol;
};
__device__ __forceinline__ SimPair sim_pair(int4 pi, int4 pj) {
  const int Dx = pj.x - pi.x, Dy = pj.y - pi.y, ex = pj.z - pi.z, ey = pj.w - pi.w;
  SimPair p;
  p.A = Dx * ex + Dy * ey, p.B = Dx * ey - Dy * ex, p.dd = Dx * Dx + Dy * Dy;
  p.fx = p.A * pi.x - p.B * pi.y - p.dd * pi.z;
  p.fy = p.A * pi.y + p.B * pi.x - p.dd * pi.w;
  p.tol = 16 * p.dd;
  return p;
}
__device__ __forceinline__ bool sim_inlier(const SimPair& p, int4 pm) {
  const int rx = __mul24(p.A, pm.x) - __mul24(p.B, pm.y) - __mul24(p.dd, pm.z) - p.fx;
  const int ry = __mul24(p.A, pm.y) + __mul24(p.B, pm.x) - __mul24(p.dd, pm.w) - p.fy;
  return ((int)(abs(rx) <= p.tol) & (int)(abs(ry) <= p.tol)) != 0;
}

__global__ __launch_bounds__(kSimThreads) void motion_sim_pairs_kernel(RowTab tab, const int* __restrict__ votes,
                                                                      int* __restrict__ sim) {
  __shared__ int4 pts[128];
  __shared__ int wcount[2];
  __shared__ unsigned long long red_key[kSimThreads / 64];
  __shared__ int red_pairs[kSimThreads / 64];
  const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = sim_gather(tab.r[row], votes + (int64_t)row * kVoteInts, pts, wcount);  // (uniform, <= 100)
  unsigned long long best = 0;
  int pairs = 0;
  for (int p = blockIdx.x * kSimThreads + tid; p < n * n; p += kSimGroups * kSimThreads) {
    const int i = p / n, j = p - i * n;
    if (i >= j) continue;
    const int4 pi = pts[i], pj = pts[j];
    const SimPair q = sim_pair(pi, pj);
    if (q.dd < 4) continue;
    pairs += 1;
    int c = 0;
#pragma unroll 4
    for (int m = 0; m < n; ++m) c += sim_inlier(q, pts[m]);
    const unsigned long long key = ((unsigned long long)c << 32) | ((unsigned)(0xffff - i) << 16) | (unsigned)(0xffff - j);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)best, m, 64), hi = __shfl_xor((unsigned)(best >> 32), m, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    best = o > best ? o : best;
    pairs += __shfl_xor(pairs, m, 64);
  }
  if (lane == 0) red_key[wave] = best, red_pairs[wave] = pairs;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < kSimThreads / 64; ++i) best = red_key[i] > best ? red_key[i] : best, pairs += red_pairs[i];
    int* slot = sim + 8 * (int64_t)gridDim.y + ((int64_t)row * kSimGroups + blockIdx.x) * kSimSlotInts;
    slot[0] = (int)(unsigned)(best >> 32), slot[1] = (int)(unsigned)best, slot[2] = pairs, slot[3] = 0;
  }
}

__global__ __launch_bounds__(kFinishThreads) void motion_sim_fit_kernel(RowTab tab, int R, int min_blocks,
                                                                       const int* __restrict__ votes,
                                                                       const int* __restrict__ sim,
                                                                       float* __restrict__ motion, int* __restrict__ diag) {
  __shared__ int4 pts[128];
  __shared__ int wcount[2];
  __shared__ unsigned long long sums[8];  // c2, sp_x, sp_y, sq_x, sq_y, sum |P|^2, sum P.Q, sum P x Q (two's complement)
  const int row = blockIdx.x, tid = threadIdx.x;
  const Row& r = tab.r[row];  // (uniform)
  const int n = sim_gather(r, votes + (int64_t)row * kVoteInts, pts, wcount);
  const int N = gridDim.x;
  const int* slots = sim + 8 * (int64_t)N + (int64_t)row * kSimGroups * kSimSlotInts;
  unsigned long long best = 0;
  int pairs = 0;
#pragma unroll
  for (int g = 0; g < kSimGroups; ++g) {  // (every thread reads the same words)
    const int* slot = slots + g * kSimSlotInts;
    const unsigned long long key = ((unsigned long long)(unsigned)slot[0] << 32) | (unsigned)slot[1];
    best = key > best ? key : best;
    pairs += slot[2];
  }
  const int bi = pairs ? 0xffff - (int)((best >> 16) & 0xffff) : -1, bj = pairs ? 0xffff - (int)(best & 0xffff) : -1;
  if (tid < 8) sums[tid] = 0;
  __syncthreads();
  if (pairs && tid < n) {
    const int4 pm = pts[tid];
    if (sim_inlier(sim_pair(pts[bi], pts[bj]), pm)) {
      const long long off = 16 * R + 128;  // P = 256 g + 16 R + 128, Q = P + v
      const long long Px = 256 * pm.x + off, Py = 256 * pm.y + off, Qx = pm.z + off, Qy = pm.w + off;
      atomicAdd(&sums[0], 1ull);
      atomicAdd(&sums[1], (unsigned long long)Px);
      atomicAdd(&sums[2], (unsigned long long)Py);
      atomicAdd(&sums[3], (unsigned long long)Qx);
      atomicAdd(&sums[4], (unsigned long long)Qy);
      atomicAdd(&sums[5], (unsigned long long)(Px * Px + Py * Py));
      atomicAdd(&sums[6], (unsigned long long)(Px * Qx + Py * Qy));
      atomicAdd(&sums[7], (unsigned long long)(Px * Qy - Py * Qx));
    }
  }
  __syncthreads();
  if (tid != 0) return;
  const long long c = (long long)sums[0], spx = (long long)sums[1], spy = (long long)sums[2], sqx = (long long)sums[3],
                  sqy = (long long)sums[4];
  const long long Sxx = c * (long long)sums[5] - (spx * spx + spy * spy);
  const long long An = c * (long long)sums[6] - (spx * sqx + spy * sqy);
  const long long Bn = c * (long long)sums[7] - (spx * sqy - spy * sqx);
  const bool valid = n >= min_blocks && pairs >= 1 && c >= min_blocks && 2 * c >= n && Sxx > 0 && 2 * An >= Sxx &&
                     An <= 2 * Sxx && 2 * (Bn < 0 ? -Bn : Bn) <= Sxx;
  const float* tm = reinterpret_cast<const float*>(sim) + 4 * (int64_t)row;  // the translation rule's row: dx, dy, valid, 0
  const int* td = sim + 4 * (int64_t)N + 4 * (int64_t)row;
  float* m = motion + 8 * (int64_t)row;
  if (valid) {
    const float den = (float)(16 * c);
    m[0] = (float)((sqx - spx) * r.k) / den, m[1] = (float)((sqy - spy) * r.k) / den, m[2] = 1.f, m[3] = 2.f;
    m[4] = (float)An / (float)Sxx, m[5] = (float)Bn / (float)Sxx;
    m[6] = (float)(spx * r.k) / den, m[7] = (float)(spy * r.k) / den;
  } else {
    const bool t = tm[2] == 1.f;
    m[0] = t ? tm[0] : 0.f, m[1] = t ? tm[1] : 0.f, m[2] = t ? 1.f : 0.f, m[3] = t ? 1.f : 0.f, m[4] = t ? 1.f : 0.f;
    m[5] = 0.f, m[6] = 0.f, m[7] = 0.f;
  }
  int* d = diag + 8 * (int64_t)row;
  d[0] = td[0], d[1] = td[1], d[2] = td[2], d[3] = td[3];
  d[4] = pairs, d[5] = pairs ? (int)(best >> 32) : 0, d[6] = bi, d[7] = bj;
}

// what the two entry points share: every argument check, then the row table and the launch extents
struct Plan {
  RowTab tab;
  int R, texture, min_blocks, bands, th_max, nb_max;
};
int plan_of(const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host, const int* stream_of_row_host,
            int64_t S, void* state_dev, const int* settings_host, void* work_dev, int64_t work_bytes, int64_t work_need,
            const void* motion_out_dev, const void* diag_out_dev, Plan& plan) {
  if (!src_dev || !rows_host || !stream_of_row_host || !state_dev || !settings_host || !work_dev || !motion_out_dev ||
      !diag_out_dev || src_bytes <= 0 || N <= 0 || S <= 0)
    return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX || S > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  const int G = settings_host[0], R = settings_host[1], texture = settings_host[2], min_blocks = settings_host[3];
  if (G < CODETR_MOTION_GRID_MIN || G > CODETR_MOTION_GRID_MAX || R < 1 || R > CODETR_MOTION_SEARCH_MAX || texture < 0 ||
      texture > CODETR_MOTION_TEXTURE_MAX || min_blocks < 1 || min_blocks > CODETR_MOTION_MAX_BLOCKS)
    return CODETR_E_BADARG;
  if (work_bytes < N * work_need || ((uintptr_t)work_dev & 3u) || ((uintptr_t)state_dev & 3u)) return CODETR_E_BADARG;
  RowTab& tab = plan.tab;
  tab = {};
  int bands = 1, th_max = 1, nb_max = 1;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t off = rows_host[3 * n], H = rows_host[3 * n + 1], W = rows_host[3 * n + 2];
    if (H <= 0 || W <= 0 || off < 0) return CODETR_E_BADARG;
    if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (off > src_bytes || H * W * 3 > src_bytes - off) return CODETR_E_BADARG;
    if (stream_of_row_host[n] < 0 || stream_of_row_host[n] >= S) return CODETR_E_BADARG;
    Row& r = tab.r[n];
    const int64_t m = H > W ? H : W;
    r.off = off, r.H = (int)H, r.W = (int)W;
    r.k = (int)((m + G - 1) / G);  // >= 1, <= 1024 (G >= 32, a side <= 32767)
    r.th = r.H / r.k, r.tw = r.W / r.k;
    r.nbx = r.tw - 2 * R > 0 ? (r.tw - 2 * R) / 16 : 0;
    r.nby = r.th - 2 * R > 0 ? (r.th - 2 * R) / 16 : 0;
    r.stream = stream_of_row_host[n];
    r.prev = -1, r.same = 0, r.last = 1;
    for (int64_t p = n - 1; p >= 0; --p)
      if (tab.r[p].stream == r.stream) {
        r.prev = (int)p, r.same = tab.r[p].H == r.H && tab.r[p].W == r.W;
        tab.r[p].last = 0;
        break;
      }
    const int cells = kBandPixels / r.k > 1 ? kBandPixels / r.k : 1;
    bands = (r.tw + cells - 1) / cells > bands ? (r.tw + cells - 1) / cells : bands;
    th_max = r.th > th_max ? r.th : th_max;
    nb_max = r.nbx * r.nby > nb_max ? r.nbx * r.nby : nb_max;
  }
  plan.R = R, plan.texture = texture, plan.min_blocks = min_blocks;
  plan.bands = bands, plan.th_max = th_max, plan.nb_max = nb_max;
  return 0;
}

// the three launches of the translation rule
void launch_translation(hipStream_t s, const Plan& plan, const void* src_dev, int64_t N, void* state_dev, void* work_dev,
                        float* motion, int* diag) {
  unsigned char* thumbs = static_cast<unsigned char*>(work_dev);
  int* votes = reinterpret_cast<int*>(thumbs + N * (int64_t)kThumbBytes);
  unsigned char* states = static_cast<unsigned char*>(state_dev);
  hipLaunchKernelGGL(motion_thumb_kernel, dim3((unsigned)plan.bands, (unsigned)plan.th_max, (unsigned)N), dim3(kThreads), 0,
                     s, static_cast<const unsigned char*>(src_dev), plan.tab, thumbs);
  hipLaunchKernelGGL(motion_match_kernel, dim3((unsigned)plan.nb_max, (unsigned)N), dim3(kThreads), 0, s, plan.tab, plan.R,
                     plan.texture, states, thumbs, votes);
  hipLaunchKernelGGL(motion_finish_kernel, dim3((unsigned)N), dim3(kFinishThreads), 0, s, plan.tab, plan.min_blocks, thumbs,
                     votes, states, motion, diag);
}

}  // namespace

extern "C" {

int codetr_motion_abi_version(void) { return CODETR_MOTION_ABI_VERSION; }
int64_t codetr_motion_state_bytes(void) { return kStateBytes; }
int64_t codetr_motion_work_bytes(int64_t N) {
  if (N <= 0 || N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_BADARG;
  return N * (int64_t)(kThumbBytes + 4 * kVoteInts);
}
int64_t codetr_motion_work2_bytes(int64_t N) {
  if (N <= 0 || N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_BADARG;
  return N * (int64_t)(kThumbBytes + 4 * kVoteInts + 4 * kSimRowInts);
}

int codetr_motion_estimate_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host,
                              const int* stream_of_row_host, int64_t S, void* state_dev, const int* settings_host,
                              void* work_dev, int64_t work_bytes, float* motion_out_dev, int* diag_out_dev) {
  Plan plan;
  if (const int rc = plan_of(src_dev, src_bytes, N, rows_host, stream_of_row_host, S, state_dev, settings_host, work_dev,
                             work_bytes, kThumbBytes + 4 * kVoteInts, motion_out_dev, diag_out_dev, plan))
    return rc;
  launch_translation(static_cast<hipStream_t>(stream), plan, src_dev, N, state_dev, work_dev, motion_out_dev, diag_out_dev);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

int codetr_motion_estimate2_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host,
                               const int* stream_of_row_host, int64_t S, void* state_dev, const int* settings_host,
                               void* work_dev, int64_t work_bytes, float* motion_out_dev, int* diag_out_dev) {
  Plan plan;
  if (const int rc = plan_of(src_dev, src_bytes, N, rows_host, stream_of_row_host, S, state_dev, settings_host, work_dev,
                             work_bytes, kThumbBytes + 4 * kVoteInts + 4 * kSimRowInts, motion_out_dev, diag_out_dev, plan))
    return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int* votes = reinterpret_cast<const int*>(static_cast<unsigned char*>(work_dev) + N * (int64_t)kThumbBytes);
  int* sim = reinterpret_cast<int*>(static_cast<unsigned char*>(work_dev) + N * (int64_t)(kThumbBytes + 4 * kVoteInts));
  launch_translation(s, plan, src_dev, N, state_dev, work_dev, reinterpret_cast<float*>(sim), sim + 4 * N);
  hipLaunchKernelGGL(motion_sim_pairs_kernel, dim3(kSimGroups, (unsigned)N), dim3(kSimThreads), 0, s, plan.tab, votes, sim);
  hipLaunchKernelGGL(motion_sim_fit_kernel, dim3((unsigned)N), dim3(kFinishThreads), 0, s, plan.tab, plan.R, plan.min_blocks,
                     votes, sim, motion_out_dev, diag_out_dev);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // extern "C"
