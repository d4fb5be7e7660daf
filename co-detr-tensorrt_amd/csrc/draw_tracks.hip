// The tracker's output on the picture (include/codetr_draw_tracks.h): the history of every track's position, kept on the
// device, and the drawing of trails, per-identity colours and ids in place in the packed RGB images.
//
// trail_update_kernel  one 256-thread workgroup per stream walks the stream's rows of the launch in row order, as
//                      track_kernel does.  The stream's whole state -- the entry table and the rings, 16 + 16 T + 4 T K bytes,
//                      in the header's layout -- sits in LDS for the launch: read once, written back once, a stream without
//                      a row is not touched.  Per row:
//   Retire   a thread per entry; a retired entry's ring is zeroed by its thread.
//   Points   a thread per detection row: key and packed point into LDS (key 0: takes no part).
//   Lookup   a wave per candidate (the key is wave-uniform): the lanes compare it with the keys of the lower rows (a
//            duplicate is dropped) and with the T ids, one ballot per 64; lane 0 appends to the entry found -- candidates
//            with different keys hit different entries, so nothing races -- or marks the candidate new.
//   Starts   the free entries and then the new candidates are ranked in index order by ballot, the count of set lower lanes
//            and a per-wave base exchanged through LDS (ordered_rank: one barrier per 256); the candidate of rank r takes
//            the r-th free entry.  No atomics.
//   Snapshot every 32-bit word of the row's snapshot by a thread stride: ids, lengths, points unrolled oldest first; the
//            bounding boxes by a thread per entry.
// draw_tracks_kernel   the gather form of draw.hip -- a 256-thread workgroup per 64 x 16 tile, four pixels per thread in
//                      registers, each pixel with one owner, so the layer order is the contract's and nothing races -- with
//                      a third list and three phases:
//   Phase 1a the T snapshot entries, 256 at a time: an entry whose bounding box grown by ceil(w / 2) meets the tile goes to
//            an ordered LDS list (uint16, at most 512).
//   Phase 1b draw.hip's edge and text lists (Q <= 1024: 1024 uint16 each), with the id-aware visibility and text length.
//   Phase 2a per listed entry, made wave-uniform so that its points come through the scalar cache: per segment a uniform
//            reject of the tile against the segment's grown box, then per pixel a 32-bit box test in front of the int64
//            products of the header's capsule test; a covered bit per pixel; ONE blend per trail.
//   Phase 2b, 2c  outlines and labels as draw.hip's, the colour and the text's prefix by the row's id.
//   A tile whose three lists are empty returns without touching the image; stores are byte-wise and only of touched pixels.
// fp32 with one rounding per operation: contraction is off for the whole file.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_draw_tracks.h"
#include "box_prims.h"
#include "draw_prims.h"
#include "draw_tracks_args.h"
#include "large_lds.h"

namespace {

using draw_tracks_args::Rows;
using draw_tracks_args::Table;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxT = CODETR_TRACK_MAX_TRACKS, kMaxQ = CODETR_POSTPROCESS_MAX_Q, kMaxK = CODETR_TRAIL_MAX_LENGTH;
static_assert(kMaxT <= 65536 && kMaxQ <= 65536, "the LDS lists hold uint16 indices");
static_assert(kTileW == 64 && kTileH == kWaves * kRowsPerThread, "a lane per column, four rows per thread");

__constant__ unsigned char d_font[CODETR_DRAW_FONT_BYTES] = {CODETR_DRAW_FONT_ROWS};

__device__ __forceinline__ int pack_point(int x, int y) { return (x & 0xffff) | (int)((unsigned)y << 16); }
__device__ __forceinline__ int point_x(int p) { return (int)(short)(p & 0xffff); }
__device__ __forceinline__ int point_y(int p) { return p >> 16; }

// For each of kN flags: the rank, among the threads of the workgroup that set it, of this thread in thread order, behind
// the n[i] already ranked; n[i] becomes the new total.  One barrier for all kN; the per-wave counts alternate between two
// slots (it), so a wave that runs ahead into the next call does not overwrite what a slower one still reads.
template <int kN>
__device__ __forceinline__ void ordered_ranks(const bool (&flag)[kN], int (&n)[kN], int (&rank)[kN],
                                              int (*cnt)[2][kWaves], int& it, int lane, int wave) {
  unsigned long long m[kN];
#pragma unroll
  for (int i = 0; i < kN; ++i) {
    m[i] = __ballot(flag[i]);
    if (lane == 0) cnt[it][i][wave] = __popcll(m[i]);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kN; ++i) {
    int base = n[i];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = cnt[it][i][w];
      if (w < wave) base += c;
      n[i] += c;
    }
    rank[i] = base + lower_lanes(m[i]);
  }
  it ^= 1;
}
__device__ __forceinline__ int ordered_rank(bool flag, int& n, int (*cnt)[2][kWaves], int& it, int lane, int wave) {
  const bool f[1] = {flag};
  int m[1] = {n}, r[1];
  ordered_ranks<1>(f, m, r, cnt, it, lane, wave);
  n = m[0];
  return r[0];
}

// ---- the trail state ---------------------------------------------------------------------------------------------------

// the state, then per detection row a key and a point (4 bytes each), the free list (2 T) and the new flags (Q)
inline int64_t trail_lds_bytes(int64_t T, int64_t K, int64_t Q) {
  return draw_tracks_args::state_bytes(T, K) + 8 * Q + (2 * T + Q + 3) / 4 * 4;
}

// grid (S), dynamic LDS trail_lds_bytes(T, K, Q)
template <class E>
__global__ __launch_bounds__(kThreads) void trail_update_kernel(const E* __restrict__ boxes, const int* __restrict__ count,
                                                                int N, int Q, Rows tab, int* __restrict__ states, int T,
                                                                int K, const int* __restrict__ ids, int retain,
                                                                int anchor, int tentative, int* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  __shared__ int s_cnt[2][2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int state_ints = 4 + 4 * T + T * K, snap_ints = 4 * T + T * K;
  int* s_hdr = lds;
  int* s_id = lds + 4;
  int* s_last = s_id + T;
  int* s_len = s_last + T;
  int* s_head = s_len + T;
  int* s_ring = s_head + T;  // [T][K] packed points
  int* s_key = lds + state_ints;  // [Q]
  int* s_pt = s_key + Q;          // [Q]
  unsigned short* s_free = (unsigned short*)(s_pt + Q);  // [T]
  unsigned char* s_new = (unsigned char*)(s_free + T);   // [Q]

  bool mine = false;  // (uniform)
  for (int n = 0; n < N; ++n) mine = mine || tab.stream[n] == (int)blockIdx.x;
  if (!mine) return;
  int* state = states + (int64_t)blockIdx.x * state_ints;
  for (int i = tid; i < state_ints; i += kThreads) lds[i] = state[i];
  __syncthreads();

  int it = 0;
  for (int n = 0; n < N; ++n) {
    if (tab.stream[n] != (int)blockIdx.x) continue;  // (uniform)
    const int f = s_hdr[0];
    const int cnt = min(max(count[n], 0), Q);
    // 1. retirement
    for (int t = tid; t < T; t += kThreads)
      if (s_id[t] != 0 && f - s_last[t] >= retain) {
        s_id[t] = s_last[t] = s_len[t] = s_head[t] = 0;
        for (int k = 0; k < K; ++k) s_ring[t * K + k] = 0;
      }
    // 2. the candidates' keys and points
    for (int j = tid; j < cnt; j += kThreads) {
      const int id = ids[(int64_t)n * Q + j];
      const E* b = boxes + ((int64_t)n * Q + j) * 4;
      const float x1 = to_f32(b[0]), y1 = to_f32(b[1]), x2 = to_f32(b[2]), y2 = to_f32(b[3]);
      const bool in = (id > 0 || (tentative && id != 0 && id != (int)0x80000000)) && finite_f(x1) && finite_f(y1) &&
                      finite_f(x2) && finite_f(y2);
      const float xs = x1 + x2, ys = y1 + y2;
      const float xa = xs * 0.5f, ya = anchor == CODETR_TRAIL_BOTTOM ? y2 : ys * 0.5f;
      s_key[j] = in ? (id < 0 ? -id : id) : 0;
      s_pt[j] = pack_point(pixel_coord(xa), pixel_coord(ya));
      s_new[j] = 0;
    }
    __syncthreads();
    // 3. a wave per candidate: duplicate of a lower row? an entry with this id?
    for (int j = wave; j < cnt; j += kWaves) {
      const int key = __builtin_amdgcn_readfirstlane(s_key[j]);
      if (key == 0) continue;
      bool dup = false;  // (uniform)
      for (int base = 0; base < j && !dup; base += 64) dup = __ballot(base + lane < j && s_key[base + lane] == key) != 0ull;
      if (dup) continue;
      int found = -1;  // (uniform)
      for (int base = 0; base < T && found < 0; base += 64) {
        const unsigned long long m = __ballot(base + lane < T && s_id[base + lane] == key);
        if (m) found = base + (int)__builtin_ctzll(m);
      }
      if (lane == 0 && found < 0) s_new[j] = 1;
      if (lane == 0 && found >= 0) {
        const int len = s_len[found], head = s_head[found];
        if (len < K) {
          s_ring[found * K + (head + len) % K] = s_pt[j];
          s_len[found] = len + 1;
        } else {
          s_ring[found * K + head] = s_pt[j];
          s_head[found] = (head + 1) % K;
        }
        s_last[found] = f;
      }
    }
    __syncthreads();
    // 4. the free entries in index order, then the new candidates in row order take them
    int nfree = 0, nnew = 0;  // (uniform)
    for (int base = 0; base < T; base += kThreads) {
      const int t = base + tid;
      const bool is_free = t < T && s_id[t] == 0;
      const int r = ordered_rank(is_free, nfree, s_cnt, it, lane, wave);
      if (is_free) s_free[r] = (unsigned short)t;
    }
    __syncthreads();
    for (int base = 0; base < cnt; base += kThreads) {
      const int j = base + tid;
      const bool is_new = j < cnt && s_new[j] != 0;
      const int r = ordered_rank(is_new, nnew, s_cnt, it, lane, wave);
      if (is_new && r < nfree) {
        const int t = s_free[r];
        s_id[t] = s_key[j];
        s_last[t] = f;
        s_len[t] = 1;
        s_head[t] = 0;
        s_ring[t * K] = s_pt[j];
      }
    }
    __syncthreads();
    // 5. the row's snapshot: ids and lengths, boxes, points oldest first
    int* o = out + (int64_t)n * snap_ints;
    for (int t = tid; t < T; t += kThreads) {
      o[t] = s_id[t];
      o[T + t] = s_len[t];
      const int len = s_len[t], head = s_head[t];
      int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
      for (int k = 0; k < len; ++k) {
        const int p = s_ring[t * K + (head + k) % K];
        const int x = point_x(p), y = point_y(p);
        x0 = k ? min(x0, x) : x, x1 = k ? max(x1, x) : x;
        y0 = k ? min(y0, y) : y, y1 = k ? max(y1, y) : y;
      }
      o[2 * T + 2 * t] = pack_point(x0, y0);
      o[2 * T + 2 * t + 1] = pack_point(x1, y1);
    }
    for (int i = tid; i < T * K; i += kThreads) {
      const int t = i / K, k = i - t * K;
      o[4 * T + i] = k < s_len[t] ? s_ring[t * K + (s_head[t] + k) % K] : 0;
    }
    __syncthreads();
    // 6.
    if (tid == 0) s_hdr[0] = f + 1;
    __syncthreads();
  }
  for (int i = tid; i < state_ints; i += kThreads) state[i] = lds[i];
}

// ---- the drawing ---------------------------------------------------------------------------------------------------------

struct TrackStyle {
  int w, A, color_by, show_id, untracked;
};

__device__ __forceinline__ unsigned abs_id(int id) { return id < 0 ? 0u - (unsigned)id : (unsigned)id; }
__device__ __forceinline__ int id_digits(unsigned v) {
  int n = 1;
  while (v >= 10u) v /= 10u, ++n;
  return n;
}
// the characters "#<|id|> " add to a label
__device__ __forceinline__ int id_prefix(int id, int show_id) { return show_id && id != 0 ? 2 + id_digits(abs_id(id)) : 0; }

// header, "Layer 0": is pixel (x, y) covered by the capsule of P0 -> P1 of width w?  q = (w * w) / 4
__device__ __forceinline__ bool capsule_covers(int x, int y, int ax, int ay, int bx, int by, int w, int q) {
  const int64_t dx = bx - ax, dy = by - ay, ex = x - ax, ey = y - ay;
  const int64_t L = dx * dx + dy * dy, t = ex * dx + ey * dy;
  if (L == 0 || t <= 0) return ex * ex + ey * ey <= q;
  if (t >= L) {
    const int64_t gx = x - bx, gy = y - by;
    return gx * gx + gy * gy <= q;
  }
  const int64_t cross = ex * dy - ey * dx;
  return cross * cross <= ((int64_t)w * w * L) / 4;
}

// grid (ceil(Wmax / 64), ceil(Hmax / 16), N)
template <class E>
__global__ __launch_bounds__(kThreads) void draw_tracks_kernel(
    unsigned char* __restrict__ buf, Table tab, const E* __restrict__ boxes, const E* __restrict__ scores,
    const int64_t* __restrict__ labels, const int* __restrict__ count, int Q, const int* __restrict__ ids,
    const int* __restrict__ trails, int T, int K, const unsigned char* __restrict__ palette,
    const unsigned char* __restrict__ names, int C, const unsigned char* __restrict__ track_palette, int P, DrawStyle st,
    TrackStyle ts) {
  __shared__ unsigned short s_trail[kMaxT], s_edge[kMaxQ], s_text[kMaxQ];
  __shared__ int s_cnt[2][2][kWaves];
  const int n = blockIdx.z;
  const draw_tracks_args::Image im = tab.img[n];
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  if (tx0 >= im.W || ty0 >= im.H) return;  // a tile beyond its image (uniform)
  const int tx1 = min(tx0 + kTileW, im.W) - 1, ty1 = min(ty0 + kTileH, im.H) - 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = st.lw / 2, b = (st.lw - 1) / 2;
  const int g = (ts.w + 1) / 2, q = ts.w * ts.w / 4;
  const E* ibox = boxes + (size_t)n * Q * 4;
  const E* iscore = scores + (size_t)n * Q;
  const int64_t* ilabel = labels + (size_t)n * Q;
  const int* iid = ids + (size_t)n * Q;
  const int cnt = min(max(count[n], 0), Q);
  // image n's snapshot: id[T], len[T], box[T] (two words), points[T][K]
  const int* snap = trails ? trails + (size_t)n * (4 * T + T * K) : nullptr;
  int it = 0;

  // ---- phase 1a: which trails reach this tile, in entry order
  int nr = 0;  // (uniform)
  if (snap)
    for (int base = 0; base < T; base += kThreads) {
      const int t = base + tid;
      bool reach = false;
      if (t < T && snap[t] != 0 && snap[T + t] >= 1) {
        const int lo = snap[2 * T + 2 * t], hi = snap[2 * T + 2 * t + 1];
        reach = point_x(lo) - g <= tx1 && point_x(hi) + g >= tx0 && point_y(lo) - g <= ty1 && point_y(hi) + g >= ty0;
      }
      const int r = ordered_rank(reach, nr, s_cnt, it, lane, wave);
      if (reach) s_trail[r] = (unsigned short)t;
    }

  // ---- phase 1b: which detections reach this tile, in ascending order
  int ne = 0, nt = 0;  // (uniform)
  for (int base = 0; base < cnt; base += kThreads) {
    const int j = base + tid;
    bool edge = false, text = false;
    if (j < cnt) {
      const float s = to_f32(iscore[j]);
      const int64_t label = ilabel[j];
      const int id = iid[j];
      const float x1 = to_f32(ibox[4 * j]), y1 = to_f32(ibox[4 * j + 1]);
      const float x2 = to_f32(ibox[4 * j + 2]), y2 = to_f32(ibox[4 * j + 3]);
      if ((id != 0 || ts.untracked) && s > st.score_thr && label >= 0 && label < C && finite_f(x1) && finite_f(y1) &&
          finite_f(x2) && finite_f(y2)) {
        const Det d{pixel_coord(x1), pixel_coord(y1), pixel_coord(x2), pixel_coord(y2)};
        if (d.x2 >= d.x1 && d.y2 >= d.y1) {
          // the band's outer rectangle meets the tile and the tile is not wholly inside the inner one
          const bool outer = d.x1 - a <= tx1 && d.x2 + a >= tx0 && d.y1 - a <= ty1 && d.y2 + a >= ty0;
          const bool inner = tx0 >= d.x1 + b + 1 && tx1 <= d.x2 - b - 1 && ty0 >= d.y1 + b + 1 && ty1 <= d.y2 - b - 1;
          edge = outer && !inner;
          if (st.draw_labels) {
            const int len = id_prefix(id, ts.show_id) + name_length(names, (int)label) + 2 + int_digits(score_tenths(s)) + 2;
            const int sc = text_scale(d, st.font_scale);
            const int ox = d.x1 + st.lw, oy = d.y1 + st.lw;
            text = ox <= tx1 && ox + (6 * len + 1) * sc - 1 >= tx0 && oy <= ty1 && oy + 9 * sc - 1 >= ty0;
          }
        }
      }
    }
    const bool flags[2] = {edge, text};
    int totals[2] = {ne, nt}, rank[2];
    ordered_ranks<2>(flags, totals, rank, s_cnt, it, lane, wave);
    ne = totals[0], nt = totals[1];
    if (edge) s_edge[rank[0]] = (unsigned short)j;
    if (text) s_text[rank[1]] = (unsigned short)j;
  }
  __syncthreads();
  if (nr == 0 && ne == 0 && nt == 0) return;

  // ---- phase 2: this thread's pixels: column x, rows y[0..3]
  const int x = tx0 + lane, yb = ty0 + wave * kRowsPerThread;
  const bool col_ok = x <= tx1;
  unsigned char* img = buf + im.offset;
  int p[kRowsPerThread][3];
  bool touched[kRowsPerThread];
#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r) {
    const int y = yb + r;
    touched[r] = false;
    p[r][0] = p[r][1] = p[r][2] = 0;
    if (col_ok && y <= ty1) {
      const unsigned char* px = img + ((size_t)y * im.W + x) * 3;
      p[r][0] = px[0];
      p[r][1] = px[1];
      p[r][2] = px[2];
    }
  }

  // ---- phase 2a: trails, one blend per trail and pixel
  for (int i = 0; i < nr; ++i) {
    const int t = __builtin_amdgcn_readfirstlane((int)s_trail[i]);
    const int id = snap[t], len = min(snap[T + t], K);
    const int* pts = snap + 4 * T + t * K;
    const unsigned ci = ((unsigned)id - 1u) % (unsigned)P;
    const int c0 = track_palette[3 * ci], c1 = track_palette[3 * ci + 1], c2 = track_palette[3 * ci + 2];
    unsigned covered = 0;
    int pa = pts[0];
    for (int s = 0; s < max(len - 1, 1); ++s) {  // (a single point: the segment P0 -> P0)
      const int pb = pts[min(s + 1, len - 1)];
      const int ax = point_x(pa), ay = point_y(pa), bx = point_x(pb), by = point_y(pb);
      pa = pb;
      const int sx0 = min(ax, bx) - g, sx1 = max(ax, bx) + g, sy0 = min(ay, by) - g, sy1 = max(ay, by) + g;
      if (sx0 > tx1 || sx1 < tx0 || sy0 > ty1 || sy1 < ty0) continue;  // the segment misses the tile (uniform)
      {  // a long diagonal: its line passes the tile's centre by more than the half diagonal + w / 2 + rounding < 42 (uniform)
        const int64_t dx = bx - ax, dy = by - ay;
        const int64_t cross = (int64_t)((tx0 + tx1) / 2 - ax) * dy - (int64_t)((ty0 + ty1) / 2 - ay) * dx;
        if (cross * cross > 42 * 42 * (dx * dx + dy * dy)) continue;
      }
      if (x < sx0 || x > sx1) continue;
#pragma unroll
      for (int r = 0; r < kRowsPerThread; ++r) {
        const int y = yb + r;
        if (y >= sy0 && y <= sy1 && !(covered >> r & 1u) && capsule_covers(x, y, ax, ay, bx, by, ts.w, q)) covered |= 1u << r;
      }
    }
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r)
      if (covered >> r & 1u) {
        p[r][0] = blend(p[r][0], c0, ts.A);
        p[r][1] = blend(p[r][1], c1, ts.A);
        p[r][2] = blend(p[r][2], c2, ts.A);
        touched[r] = true;
      }
  }

  // ---- phase 2b: outlines, the colour by the row's id
  for (int i = 0; i < ne; ++i) {
    const int j = __builtin_amdgcn_readfirstlane((int)s_edge[i]);
    const Det d = pixel_box(ibox + 4 * j);
    const int label = (int)ilabel[j], id = iid[j];
    const bool by_track = ts.color_by == CODETR_COLOR_BY_TRACK && id != 0;
    const unsigned char* c = by_track ? track_palette + 3 * ((abs_id(id) - 1u) % (unsigned)P) : palette + 3 * label;
    const int c0 = c[0], c1 = c[1], c2 = c[2];
    if (x < d.x1 - a || x > d.x2 + a) continue;
    const bool x_inner = x >= d.x1 + b + 1 && x <= d.x2 - b - 1;
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
      const int y = yb + r;
      const bool on = y >= d.y1 - a && y <= d.y2 + a && !(x_inner && y >= d.y1 + b + 1 && y <= d.y2 - b - 1);
      if (on) {
        p[r][0] = blend(p[r][0], c0, st.A);
        p[r][1] = blend(p[r][1], c1, st.A);
        p[r][2] = blend(p[r][2], c2, st.A);
        touched[r] = true;
      }
    }
  }

  // ---- phase 2c: labels, "#<id> " in front while the row has a track
  for (int i = 0; i < nt; ++i) {
    const int j = __builtin_amdgcn_readfirstlane((int)s_text[i]);
    const Det d = pixel_box(ibox + 4 * j);
    const int label = (int)ilabel[j], id = iid[j];
    const int tenths = score_tenths(to_f32(iscore[j]));
    const unsigned char* name = names + (size_t)label * kNameRow;
    const int nlen = name_length(names, label), nd = int_digits(tenths);
    const int pre = id_prefix(id, ts.show_id);
    const int len = pre + nlen + 2 + nd + 2;
    const int sc = text_scale(d, st.font_scale);
    const int gx = x - (d.x1 + st.lw);
    if (gx < 0 || gx >= (6 * len + 1) * sc) continue;
    const int fx = gx / sc;
    // the character of this column and the bit of its glyph row that the column shows (none between characters)
    int k = fx >= 1 ? (fx - 1) / 6 : 0;
    const int col = fx >= 1 ? (fx - 1) - 6 * k : 5;
    int ch;
    if (k < pre) {  // '#' or '~', the digits of |id| from the highest, a space
      if (k == 0) ch = id < 0 ? '~' : '#';
      else if (k == pre - 1) ch = ' ';
      else {
        unsigned v = abs_id(id);
        for (int z = pre - 2 - k; z > 0; --z) v /= 10u;
        ch = '0' + (int)(v % 10u);
      }
    } else if ((k -= pre) < nlen) {
      ch = name[1 + k];
    } else {
      const int t = k - nlen;  // ": " then the integer part, ".", the tenth
      const int whole = tenths / 10;
      if (t == 0) ch = ':';
      else if (t == 1) ch = ' ';
      else if (t == 2 + nd) ch = '.';
      else if (t == 3 + nd) ch = '0' + tenths % 10;
      else {
        const int pos = nd - 1 - (t - 2);  // 0 = units
        ch = '0' + (pos == 0 ? whole % 10 : pos == 1 ? (whole / 10) % 10 : whole / 100);
      }
    }
    if (ch < 32 || ch > 126) ch = '?';
    const unsigned char* glyph = d_font + (ch - 32) * 7;
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
      const int y = yb + r;
      const int gy = y - (d.y1 + st.lw);
      if (gy < 0 || gy >= 9 * sc) continue;
      const int fy = gy / sc;
      const bool ink = col < 5 && fy >= 1 && fy <= 7 && ((glyph[fy >= 1 && fy <= 7 ? fy - 1 : 0] >> (4 - col)) & 1);
      if (ink) {
        p[r][0] = st.text[0];
        p[r][1] = st.text[1];
        p[r][2] = st.text[2];
      } else {
        p[r][0] = blend(p[r][0], 0, st.A);
        p[r][1] = blend(p[r][1], 0, st.A);
        p[r][2] = blend(p[r][2], 0, st.A);
      }
      touched[r] = true;
    }
  }

#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r) {
    const int y = yb + r;
    if (touched[r] && col_ok && y <= ty1) {
      unsigned char* px = img + ((size_t)y * im.W + x) * 3;
      px[0] = (unsigned char)p[r][0];
      px[1] = (unsigned char)p[r][1];
      px[2] = (unsigned char)p[r][2];
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

template <class E>
int launch_trail_update(void* stream, const void* boxes, const int* count, int64_t N, int64_t Q, const int* stream_of_row,
                        int64_t S, void* state, int64_t T, int64_t K, const int* ids, int64_t retain, int anchor,
                        int tentative, void* out) {
  Rows rows;
  if (const int rc = draw_tracks_args::check_update(boxes, count, N, Q, stream_of_row, S, state, T, K, ids, retain, anchor,
                                                    tentative, out, &rows))
    return rc;
  constexpr auto kernel = trail_update_kernel<E>;
  const int64_t lds = trail_lds_bytes(T, K, Q);
  if (lds + 1024 > 64 * 1024)  // (the opt-in is needed once dynamic + static LDS pass 64 KB)
    if (const hipError_t err = allow_large_lds<kernel>((int)trail_lds_bytes(kMaxT, kMaxK, kMaxQ)); err != hipSuccess)
      return (int)err;
  hipLaunchKernelGGL(kernel, dim3((unsigned)S), dim3(kThreads), (size_t)lds, static_cast<hipStream_t>(stream),
                     static_cast<const E*>(boxes), count, (int)N, (int)Q, rows, static_cast<int*>(state), (int)T, (int)K,
                     ids, (int)(retain > 0x7fffffffLL ? 0x7fffffffLL : retain), anchor, tentative, static_cast<int*>(out));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

template <class E>
int launch_draw_tracks(void* stream, void* buf, int64_t buf_bytes, int64_t N, const int64_t* images, const void* boxes,
                       const void* scores, const int64_t* labels, const int* count, int64_t Q,
                       const unsigned char* palette, const unsigned char* names, int64_t C, int line_width, float alpha,
                       float score_thr, uint32_t text_rgb, int font_scale, int draw_labels, const int* ids,
                       const void* trails, int64_t T, int64_t K, const unsigned char* track_palette, int64_t P,
                       int trail_width, float trail_alpha, int color_by, int show_id, int untracked) {
  Table tab = {};
  int64_t Hmax = 0, Wmax = 0;
  if (const int rc = draw_tracks_args::check_draw(buf, buf_bytes, N, images, boxes, scores, labels, count, Q, palette, names,
                                                  C, line_width, alpha, score_thr, text_rgb, font_scale, draw_labels, ids,
                                                  trails, T, K, track_palette, P, trail_width, trail_alpha, color_by,
                                                  show_id, untracked, &tab, &Hmax, &Wmax))
    return rc;
  DrawStyle st;
  st.lw = line_width;
  st.A = (int)(alpha * 256.0f + 0.5f);
  st.font_scale = font_scale;
  st.draw_labels = draw_labels;
  st.score_thr = score_thr;
  st.text[0] = (int)((text_rgb >> 16) & 255u);
  st.text[1] = (int)((text_rgb >> 8) & 255u);
  st.text[2] = (int)(text_rgb & 255u);
  const TrackStyle ts = {trail_width, (int)(trail_alpha * 256.0f + 0.5f), color_by, show_id, untracked};
  const dim3 grid((unsigned)((Wmax + kTileW - 1) / kTileW), (unsigned)((Hmax + kTileH - 1) / kTileH), (unsigned)N);
  hipLaunchKernelGGL((draw_tracks_kernel<E>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned char*>(buf), tab, static_cast<const E*>(boxes), static_cast<const E*>(scores),
                     labels, count, (int)Q, ids, static_cast<const int*>(trails), trails ? (int)T : 0, trails ? (int)K : 0,
                     palette, names, (int)C, track_palette, (int)P, st, ts);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

extern "C" {

int codetr_draw_tracks_abi_version(void) { return CODETR_DRAW_TRACKS_ABI_VERSION; }

int64_t codetr_trail_state_bytes(int64_t max_tracks, int64_t length) {
  if (!draw_tracks_args::trail_shape_ok(max_tracks, length)) return CODETR_E_BADARG;
  return draw_tracks_args::state_bytes(max_tracks, length);
}

int64_t codetr_trail_snapshot_bytes(int64_t max_tracks, int64_t length) {
  if (!draw_tracks_args::trail_shape_ok(max_tracks, length)) return CODETR_E_BADARG;
  return draw_tracks_args::snapshot_bytes(max_tracks, length);
}

#define CODETR_DRAW_TRACKS_ENTRIES(SUFFIX, TYPE)                                                                          \
  int codetr_trail_update_##SUFFIX(void* stream, const void* boxes_dev, const void* scores_dev, const int64_t* labels_dev, \
                                   const int* count_dev, int64_t N, int64_t Q, const int* stream_of_row_host, int64_t S,   \
                                   void* state_dev, int64_t max_tracks, int64_t length, const int* track_ids_dev,          \
                                   int64_t retain, int anchor, int tentative, void* trails_out_dev) {                      \
    (void)scores_dev, (void)labels_dev;                                                                                    \
    return launch_trail_update<TYPE>(stream, boxes_dev, count_dev, N, Q, stream_of_row_host, S, state_dev, max_tracks,     \
                                     length, track_ids_dev, retain, anchor, tentative, trails_out_dev);                    \
  }                                                                                                                        \
  int codetr_draw_tracks_##SUFFIX(                                                                                         \
      void* stream, void* buf_dev, int64_t buf_bytes, int64_t N, const int64_t* images_host, const void* boxes_dev,        \
      const void* scores_dev, const int64_t* labels_dev, const int* count_dev, int64_t Q, const unsigned char* palette_dev, \
      const unsigned char* names_dev, int64_t C, int line_width, float alpha, float score_thr, uint32_t text_rgb,          \
      int font_scale, int draw_labels, const int* track_ids_dev, const void* trails_dev, int64_t max_tracks,               \
      int64_t length, const unsigned char* track_palette_dev, int64_t P, int trail_width, float trail_alpha, int color_by, \
      int show_id, int untracked) {                                                                                        \
    return launch_draw_tracks<TYPE>(stream, buf_dev, buf_bytes, N, images_host, boxes_dev, scores_dev, labels_dev,         \
                                    count_dev, Q, palette_dev, names_dev, C, line_width, alpha, score_thr, text_rgb,       \
                                    font_scale, draw_labels, track_ids_dev, trails_dev, max_tracks, length,                \
                                    track_palette_dev, P, trail_width, trail_alpha, color_by, show_id, untracked);         \
  }
CODETR_DRAW_TRACKS_ENTRIES(f16, _Float16)
CODETR_DRAW_TRACKS_ENTRIES(bf16, Bf16)
CODETR_DRAW_TRACKS_ENTRIES(f32, float)
#undef CODETR_DRAW_TRACKS_ENTRIES

}  // extern "C"
