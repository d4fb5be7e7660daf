// Camera-motion estimate for the tracker: codetr_motion_estimate_u8 of include/codetr_motion.h, which states the rule
// operation by operation (integers, one fp32 division per axis at the end); this file follows that text.  Three launches
// on the caller's stream, nothing host-visible in between; the thumbnails and the votes live in the caller's scratch.
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

}  // namespace

extern "C" {

int codetr_motion_abi_version(void) { return CODETR_MOTION_ABI_VERSION; }
int64_t codetr_motion_state_bytes(void) { return kStateBytes; }
int64_t codetr_motion_work_bytes(int64_t N) {
  if (N <= 0 || N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_BADARG;
  return N * (int64_t)(kThumbBytes + 4 * kVoteInts);
}

int codetr_motion_estimate_u8(void* stream, const void* src_dev, int64_t src_bytes, int64_t N, const int64_t* rows_host,
                              const int* stream_of_row_host, int64_t S, void* state_dev, const int* settings_host,
                              void* work_dev, int64_t work_bytes, float* motion_out_dev, int* diag_out_dev) {
  if (!src_dev || !rows_host || !stream_of_row_host || !state_dev || !settings_host || !work_dev || !motion_out_dev ||
      !diag_out_dev || src_bytes <= 0 || N <= 0 || S <= 0)
    return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX || S > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  const int G = settings_host[0], R = settings_host[1], texture = settings_host[2], min_blocks = settings_host[3];
  if (G < CODETR_MOTION_GRID_MIN || G > CODETR_MOTION_GRID_MAX || R < 1 || R > CODETR_MOTION_SEARCH_MAX || texture < 0 ||
      texture > CODETR_MOTION_TEXTURE_MAX || min_blocks < 1 || min_blocks > CODETR_MOTION_MAX_BLOCKS)
    return CODETR_E_BADARG;
  if (work_bytes < N * (int64_t)(kThumbBytes + 4 * kVoteInts) || ((uintptr_t)work_dev & 3u) || ((uintptr_t)state_dev & 3u))
    return CODETR_E_BADARG;
  RowTab tab = {};
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
  unsigned char* thumbs = static_cast<unsigned char*>(work_dev);
  int* votes = reinterpret_cast<int*>(thumbs + N * (int64_t)kThumbBytes);
  unsigned char* states = static_cast<unsigned char*>(state_dev);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(motion_thumb_kernel, dim3((unsigned)bands, (unsigned)th_max, (unsigned)N), dim3(kThreads), 0, s,
                     static_cast<const unsigned char*>(src_dev), tab, thumbs);
  hipLaunchKernelGGL(motion_match_kernel, dim3((unsigned)nb_max, (unsigned)N), dim3(kThreads), 0, s, tab, R, texture,
                     states, thumbs, votes);
  hipLaunchKernelGGL(motion_finish_kernel, dim3((unsigned)N), dim3(kFinishThreads), 0, s, tab, min_blocks, thumbs, votes,
                     states, motion_out_dev, diag_out_dev);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // extern "C"
