// The tracker's device code and argument checks (track.hip holds the one kernel, its launcher and the entry points): the
// LDS layout, the pair value, the greedy association (the rule of codetr_hip.h) and the optimal one (codetr_assign.h), the
// appearance cue (codetr_appearance.h), the walk over a stream's frames with the association left to the caller, and the
// argument checks of the launcher.
// fp32 with one rounding per operation: contraction is off for everything below, divisions are IEEE.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assign_core.h"
#include "box_prims.h"
#include "codetr_appearance.h"
#include "codetr_hip.h"
#include "codetr_motion.h"
#include "large_lds.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kOwn = CODETR_TRACK_MAX_TRACKS / kThreads;  // tracks a thread owns in a matching phase
constexpr int kNone = 0x7fffffff;
constexpr int kStaticLds = 1024;  // an upper bound of what the compiler adds for the workgroup votes (256 bytes today)
static_assert(CODETR_TRACK_MAX_TRACKS % kThreads == 0, "a whole number of tracks per thread");

struct RowTable {  // a kernel argument, like prepost.hip's BatchTable: the stream of every row
  int stream[CODETR_PREPROCESS_BATCH_MAX];
};
struct Settings {
  float obj_high, obj_low, init_thr, match_high, match_low, match_tentative;
  int retain, tentatives, weight_iou;
};

constexpr float kWp = 1.0f / 20.0f, kWv = 1.0f / 160.0f;

// position / velocity standard deviation of coordinate c (0 cx, 1 cy, 2 a, 3 h) at height h
__device__ __forceinline__ float std_p(int c, float h) { return c == 2 ? 1e-2f : kWp * h; }
__device__ __forceinline__ float std_v(int c, float h) { return c == 2 ? 1e-5f : kWv * h; }

// the workgroup's LDS, carved from one dynamic buffer
struct Lds {
  // the state, in the header's order
  int* hdr;            // [4] f, issued, refused, 0
  long long* label;    // [T]
  int *id, *hits, *tent, *last;  // [T]
  float* mean;         // [8][T]   (c * 2 + {p, v})
  float* cov;          // [12][T]  (c * 3 + {A, B, C})
  // working arrays
  float4* tbox;        // [T] the predicted box of a live track
  int* match;          // [T] the candidate a track took in this frame, -1: none
  unsigned short* freelist;  // [T]
  float4* cbox;        // [Q]
  long long* clabel;   // [Q]
  float* cscore;       // [Q]
  int* out;            // [Q]
  unsigned char* cls;  // [Q] 0: takes no part or taken, 1: high and free, 2: low and free
  float* red_v;        // [2][kWaves]
  int *red_t, *red_j;  // [2][kWaves]
  int* wsum;           // [kWaves]
};

__host__ __device__ inline int64_t state_bytes_of(int64_t T) { return 16 + 104 * T; }
__host__ __device__ inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }
__host__ __device__ inline int64_t lds_bytes_of(int64_t T, int64_t Q) {
  return round16(state_bytes_of(T)) + 24 * T + 32 * Q + round16(Q) + 32 * kWaves;
}

__device__ __forceinline__ Lds carve(unsigned char* base, int T, int Q) {
  Lds s;
  unsigned char* p = base;
  s.hdr = (int*)p, p += 16;
  s.label = (long long*)p, p += 8 * T;
  s.id = (int*)p, p += 4 * T;
  s.hits = (int*)p, p += 4 * T;
  s.tent = (int*)p, p += 4 * T;
  s.last = (int*)p, p += 4 * T;
  s.mean = (float*)p, p += 32 * T;
  s.cov = (float*)p;
  p = base + round16(state_bytes_of(T));  // the 16-byte items first, then 8, 4, 2 and 1
  s.tbox = (float4*)p, p += 16 * T;
  s.cbox = (float4*)p, p += 16 * Q;
  s.clabel = (long long*)p, p += 8 * Q;
  s.match = (int*)p, p += 4 * T;
  s.cscore = (float*)p, p += 4 * Q;
  s.out = (int*)p, p += 4 * Q;
  s.red_v = (float*)p, p += 8 * kWaves;
  s.red_t = (int*)p, p += 8 * kWaves;
  s.red_j = (int*)p, p += 8 * kWaves;
  s.wsum = (int*)p, p += 8 * kWaves;
  s.freelist = (unsigned short*)p, p += 4 * T;  // (2 T used)
  s.cls = p;
  return s;
}

// (v, j) of the better of two bests: the higher value, ties to the lower j; j == kNone: no candidate
__device__ __forceinline__ void take_better(float& v, int& j, float ov, int oj) {
  if (oj != kNone && (j == kNone || ov > v || (ov == v && oj < j))) v = ov, j = oj;
}

// the best free candidate of class `cls` for track t, by the whole wave (t is wave-uniform): lanes stride over the
// candidates, then one wave arg-max.  `skip`: a candidate taken so recently that its cls byte may not be visible yet.
// kApp (codetr_appearance.h): `add` is the track's row of appearance addends, one per candidate, added to the value.
template <bool kApp = false>
__device__ __forceinline__ void wave_best(const Lds& s, int t, int cnt, int cls, bool weighted, float thr, int skip,
                                          int lane, float& best_v, int& best_j, const float* add = nullptr) {
  const float4 tb = s.tbox[t];
  const float ta = box_area(tb);
  const long long tl = s.label[t];
  float bv = 0.f;
  int bj = kNone;
  for (int j = lane; j < cnt; j += 64) {
    if (s.cls[j] != cls || j == skip || s.clabel[j] != tl) continue;
    const float4 cb = s.cbox[j];
    const float iou = box_iou(tb, ta, cb, box_area(cb));
    float val = weighted ? iou * s.cscore[j] : iou;
    if constexpr (kApp) val = val + add[j];
    if (val >= thr && (bj == kNone || val > bv)) bv = val, bj = j;  // (a NaN compares false; ascending j: ties keep the lower)
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float ov = __shfl_xor(bv, m, 64);
    const int oj = __shfl_xor(bj, m, 64);
    take_better(bv, bj, ov, oj);
  }
  best_v = bv, best_j = bj;
}

// exclusive rank of `flag` among the workgroup's threads in tid order + the total; two barriers (the second frees wsum)
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int lane, int wave, int& total) {
  const unsigned long long b = __ballot(flag);
  const int r = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = wsum[w];
    before += w < wave ? c : 0;
    all += c;
  }
  __syncthreads();
  total = all;
  return before + r;
}

// one greedy association (steps 3 to 5 of the rule).  kind 0: confirmed tracks, 1: tentative tracks, 2: confirmed tracks
// matched in the previous frame.  Ends with a barrier.  kApp: `add` [T][pitch], the stream's appearance addends.
template <bool kApp = false>
__device__ __forceinline__ void match_phase(const Lds& s, int T, int cnt, int f, int kind, int cls, bool weighted, float thr,
                                            int tid, const float* add = nullptr, int pitch = 0) {
  const int lane = tid & 63, wave = tid >> 6;
  float bv[kOwn];
  int bj[kOwn];
  bool any = false;
#pragma unroll
  for (int k = 0; k < kOwn; ++k) {
    const int t = tid + k * kThreads;
    bool elig = false;
    if (t < T && s.id[t] != 0 && s.match[t] < 0) {
      const bool tent = s.tent[t] != 0;
      elig = kind == 1 ? tent : (!tent && (kind == 0 || s.last[t] == f - 1));
    }
    bv[k] = 0.f, bj[k] = kNone;
    unsigned long long need = __ballot(elig);
    while (need) {  // (wave-uniform)
      const int l = __ffsll((long long)need) - 1;
      need &= need - 1;
      float v;
      int j;
      const int wt = wave * 64 + l + k * kThreads;
      wave_best<kApp>(s, wt, cnt, cls, weighted, thr, -1, lane, v, j, kApp ? add + (int64_t)wt * pitch : nullptr);
      if (lane == l) bv[k] = v, bj[k] = j;
    }
    any |= elig;
  }
  if (__syncthreads_or(any) == 0) return;
  for (int buf = 0;; buf ^= 1) {
    // the workgroup's best pair: the highest value, ties to the lowest slot (a track's own best is its lowest j)
    float v = 0.f;
    int t = kNone, j = kNone;
#pragma unroll
    for (int k = 0; k < kOwn; ++k)  // (ascending slot: a tie keeps the lower)
      if (bj[k] != kNone && (t == kNone || bv[k] > v)) v = bv[k], t = tid + k * kThreads, j = bj[k];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const float ov = __shfl_xor(v, m, 64);
      const int ot = __shfl_xor(t, m, 64), oj = __shfl_xor(j, m, 64);
      if (ot != kNone && (t == kNone || ov > v || (ov == v && ot < t))) v = ov, t = ot, j = oj;
    }
    if (lane == 0) s.red_v[buf * kWaves + wave] = v, s.red_t[buf * kWaves + wave] = t, s.red_j[buf * kWaves + wave] = j;
    __syncthreads();
    v = 0.f, t = kNone, j = kNone;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const float ov = s.red_v[buf * kWaves + w];
      const int ot = s.red_t[buf * kWaves + w], oj = s.red_j[buf * kWaves + w];
      if (ot != kNone && (t == kNone || ov > v || (ov == v && ot < t))) v = ov, t = ot, j = oj;
    }
    if (t == kNone) break;  // (uniform)
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      const bool mine = t == tid + k * kThreads;
      if (mine) {
        s.match[t] = j;
        s.cls[j] = 0;  // taken: seen by the other waves after the next barrier, skipped by name until then
        bj[k] = kNone;
      }
      unsigned long long need = __ballot(!mine && bj[k] == j);
      while (need) {
        const int l = __ffsll((long long)need) - 1;
        need &= need - 1;
        float nv;
        int nj;
        const int wt = wave * 64 + l + k * kThreads;
        wave_best<kApp>(s, wt, cnt, cls, weighted, thr, j, lane, nv, nj, kApp ? add + (int64_t)wt * pitch : nullptr);
        if (lane == l) bv[k] = nv, bj[k] = nj;
      }
    }
  }
  __syncthreads();
}

// ---- the optimal association of codetr_assign.h: the procedure of assign_core.h over the integer gains of the header,
// computed on the fly from the boxes in LDS (no T x Q matrix).  The solver's LDS (8 T + 12 max(T, Q) + 96 bytes) lies
// behind the tracker's: 114 KB together at T = 512, Q = 1024. ----
static_assert(CODETR_TRACK_MAX_TRACKS <= CODETR_ASSIGN_MAX_ROWS && CODETR_POSTPROCESS_MAX_Q <= CODETR_ASSIGN_MAX_COLS,
              "the tracker's largest problem fits the solver");

__host__ __device__ inline int64_t lds2_offset(int64_t T, int64_t Q) { return round16(lds_bytes_of(T, Q)); }
__host__ __device__ inline int64_t lds2_bytes_of(int64_t T, int64_t Q) {
  return lds2_offset(T, Q) + assign_lds_bytes(T, T > Q ? T : Q);
}

// one optimal association (steps 3 to 5 of the rule under CODETR_ASSOCIATION_OPTIMAL); kind and cls as match_phase.  The
// phase's tracks with an eligible pair are found as the greedy phase finds its first bests (a wave per track, lanes over
// the candidates) and compacted in slot order into the free-slot list (unused until step 8); the columns are all
// candidates of the frame.  Ends with a barrier.  kApp: `add` [T][pitch], the stream's appearance addends.
template <bool kApp = false>
__device__ __forceinline__ void assign_phase(const Lds& s, const AssignLds& a, int T, int cnt, int f, int kind, int cls,
                                             bool weighted, float thr, int tid, const float* add = nullptr,
                                             int pitch = 0) {
  const int lane = tid & 63, wave = tid >> 6;
  int R = 0;  // rows: the phase's tracks with at least one eligible pair, in ascending slot order
#pragma unroll
  for (int k = 0; k < kOwn; ++k) {
    const int t = tid + k * kThreads;
    bool elig = false;
    if (t < T && s.id[t] != 0 && s.match[t] < 0) {
      const bool tent = s.tent[t] != 0;
      elig = kind == 1 ? tent : (!tent && (kind == 0 || s.last[t] == f - 1));
    }
    bool has = false;
    unsigned long long need = __ballot(elig);
    while (need) {  // (wave-uniform, at most 64 turns)
      const int l = __ffsll((long long)need) - 1;
      need &= need - 1;
      float v;
      int j;
      const int wt = wave * 64 + l + k * kThreads;
      wave_best<kApp>(s, wt, cnt, cls, weighted, thr, -1, lane, v, j, kApp ? add + (int64_t)wt * pitch : nullptr);
      if (lane == l) has = j != kNone;
    }
    int tot;
    const int r = R + block_rank(has, s.wsum, lane, wave, tot);
    if (has) s.freelist[r] = (unsigned short)t;
    R += tot;
  }
  __syncthreads();
  if (R == 0) return;  // (uniform)
  const int M = max(R, cnt);
  const auto gain_of = [&](int r, int j) -> int {
    if (j >= cnt || s.cls[j] != cls) return 0;  // (virtual, of another class, taken, or taking no part)
    const int t = s.freelist[r];
    if (s.clabel[j] != s.label[t]) return 0;
    const float4 tb = s.tbox[t], cb = s.cbox[j];
    const float iou = box_iou(tb, box_area(tb), cb, box_area(cb));
    float val = weighted ? iou * s.cscore[j] : iou;
    if constexpr (kApp) val = val + add[(int64_t)t * pitch + j];
    return val >= thr ? 1 + (int)(fminf(val - thr, 2.0f) * 1048576.0f) : 0;  // (a NaN compares false)
  };
  assign_solve(a, R, M, gain_of, tid);
  for (int j = tid; j < cnt; j += kThreads) {
    const int o = a.owner[j];
    if (o >= 0 && gain_of(o, j) > 0) {
      s.match[s.freelist[o]] = j;
      s.cls[j] = 0;  // taken (only this thread reads cls[j] in this loop)
    }
  }
  __syncthreads();
}

// ---- the appearance cue of codetr_appearance.h (codetr_track_update5_*) ----
struct App {
  const unsigned short* desc = nullptr;  // [N, Q, 128] descriptors, 16-byte aligned; null: no cue
  unsigned* g = nullptr;                 // [S][T][64] the appearance states, two uint16 per word
  float* add = nullptr;                  // [S][T][Q] scratch: the addend of every pair
  float thr = 0.f, prox = 0.f, gate = 0.f;
};
constexpr int kAppFreed = -2, kAppStarted = -3;  // s.match of a slot freed (step 7) / started by candidate j: kAppStarted - j

// The addends of a frame, a wave per live track: lanes stride over the candidates and compute the gate; a gated lane then
// walks its candidate's 128 bins against the track's, which the wave holds two per lane (read lane by lane).  Every
// j < cnt of a live track is written: s where it is added, 0 elsewhere.  Only `high` candidates of the track's label are
// gated: the associations look at no other pair.  Ends with a barrier.
__device__ __forceinline__ void app_addends(const Lds& s, const App& app, int b, int n, int T, int Q, int cnt, int f,
                                            int lane, int wave) {
  const float gate2 = app.gate * app.gate;
  for (int t = wave; t < T; t += kWaves) {  // (wave-uniform)
    if (s.id[t] == 0) continue;
    const float4 tb = s.tbox[t];
    const float ta = box_area(tb);
    const long long tl = s.label[t];
    const float cx = s.mean[t], cy = s.mean[2 * T + t], a = s.mean[4 * T + t], hh = s.mean[6 * T + t];
    const bool lost = s.tent[t] == 0 && s.last[t] != f - 1 && app.gate > 0.f;
    const float wt = a * hh;
    const float r2 = gate2 * (wt * wt + hh * hh);
    const int g32 = (int)app.g[((int64_t)b * T + t) * 64 + lane];
    float* row = app.add + ((int64_t)b * T + t) * Q;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
      const int j = j0 + lane;
      bool need = false;
      if (j < cnt && s.cls[j] == 1 && s.clabel[j] == tl) {
        const float4 cb = s.cbox[j];
        const float iou = box_iou(tb, ta, cb, box_area(cb));
        need = iou >= app.prox;  // (a NaN compares false)
        if (lost) {
          const float dx = (cb.x + cb.z) * 0.5f - cx, dy = (cb.y + cb.w) * 0.5f - cy;
          const float d2 = dx * dx + dy * dy;
          need = need || d2 <= r2;
        }
      }
      float addend = 0.f;
      if (need) {
        const uint4* dp = reinterpret_cast<const uint4*>(app.desc + ((int64_t)n * Q + j) * 128);
        int I = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const uint4 d4 = dp[q];
          const unsigned d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned gk = (unsigned)__builtin_amdgcn_readlane(g32, 4 * q + e);
            I += (int)min(gk & 0xffffu, (d[e] & 0xffffu) << 4) + (int)min(gk >> 16, (d[e] >> 16) << 4);
          }
        }
        const float sim = (float)I / 8192.0f;
        addend = sim >= app.thr ? sim : 0.f;
      }
      if (j < cnt) row[j] = addend;
    }
  }
  __syncthreads();
}

// Steps 6 to 8 of the cue, a wave per slot, two bins per lane: a track matched to a `high` candidate blends (or, all zero,
// takes) its descriptor, a freed slot is zeroed, a started track takes its candidate's.  Ends with a barrier, which also
// orders these stores before the next frame's reads.
__device__ __forceinline__ void app_update(const Lds& s, const App& app, int b, int n, int T, int Q, float obj_high,
                                           int lane, int wave) {
  const unsigned* desc32 = reinterpret_cast<const unsigned*>(app.desc);
  for (int t = wave; t < T; t += kWaves) {  // (wave-uniform)
    const int m = s.match[t];
    unsigned* gp = app.g + ((int64_t)b * T + t) * 64 + lane;
    if (m == kAppFreed) {
      *gp = 0u;
    } else if (m <= kAppStarted || (m >= 0 && s.cscore[m] > obj_high)) {
      const int j = m >= 0 ? m : kAppStarted - m;
      const unsigned d = desc32[((int64_t)n * Q + j) * 64 + lane];
      const unsigned dlo = ((d & 0xffffu) << 4) & 0xffffu, dhi = ((d >> 16) << 4) & 0xffffu;
      unsigned out = dlo | (dhi << 16);
      if (m >= 0) {
        const unsigned g = *gp;
        if (__ballot(g != 0u) != 0ull) {
          const unsigned lo = (7u * (g & 0xffffu) + ((d & 0xffffu) << 4) + 4u) >> 3;
          const unsigned hi = (7u * (g >> 16) + ((d >> 16) << 4) + 4u) >> 3;
          out = (lo & 0xffffu) | (hi << 16);
        }
      }
      *gp = out;
    }
  }
  __syncthreads();
}

// One stream's rows of a launch, walked in row order (the kernel's body).  `associate(s, cnt, f)`
// runs steps 3 to 5 on the frame's candidates and predicted tracks and ends with a barrier.  kMotion (codetr_motion.h):
// 1: `motion` [N, 4] = dx, dy, valid, 0 per row, or null; a valid, finite motion is added to the predicted centres.
// 2: `motion` [N, 8] = dx, dy, valid, model, a, b, px, py per row, or null; by the model a similarity about (px, py) moves
// the predicted centres, their velocities and the height (codetr_track_update4_*), or the translation is added as under 1.
// kApp (codetr_appearance.h; `app.desc` non-null): after step 2 a pre-pass writes the appearance addend of every pair the
// first two associations can evaluate into `app.add`, and after step 8 the appearances of the stream's slots are blended,
// zeroed or started in global memory; s.match carries what happened to a slot (kAppFreed, kAppStarted - j) to that pass.
template <int kMotion = 0, bool kApp = false, class T, class Assoc>
__device__ __forceinline__ void track_stream(unsigned char* lds_raw, const T* __restrict__ boxes,
                                             const T* __restrict__ scores, const int64_t* __restrict__ labels,
                                             const int* __restrict__ count, int N, int Q, const RowTable& tab,
                                             unsigned char* __restrict__ states, int maxT, const Settings& cfg,
                                             int* __restrict__ ids_out, Assoc associate,
                                             const float* __restrict__ motion = nullptr, const App& app = App{}) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  bool have = false;
  for (int n = 0; n < N; ++n) have |= tab.stream[n] == b;  // (uniform)
  if (!have) return;  // a stream without a row in this launch keeps its state bytes

  const Lds s = carve(lds_raw, maxT, Q);
  const int64_t sbytes = state_bytes_of(maxT);
  {  // the state is one run of dwords in both places
    const unsigned* g = reinterpret_cast<const unsigned*>(states + (int64_t)b * sbytes);
    unsigned* l = reinterpret_cast<unsigned*>(lds_raw);
    for (int64_t i = tid; i < sbytes / 4; i += kThreads) l[i] = g[i];
  }
  __syncthreads();
  int f = s.hdr[0], issued = s.hdr[1], refused = s.hdr[2];  // (uniform, kept in registers over the frames)

  for (int n = 0; n < N; ++n) {
    if (tab.stream[n] != b) continue;  // (uniform)
    const int cnt = min(max(count[n], 0), Q);

    // 1. candidates
    for (int j = tid; j < Q; j += kThreads) {
      unsigned char cls = 0;
      if (j < cnt) {
        const T* bp = boxes + ((int64_t)n * Q + j) * 4;
        const float4 cb = make_float4(to_f32(bp[0]), to_f32(bp[1]), to_f32(bp[2]), to_f32(bp[3]));
        const float sc = to_f32(scores[(int64_t)n * Q + j]);
        const bool finite = __builtin_isfinite(cb.x) && __builtin_isfinite(cb.y) && __builtin_isfinite(cb.z) &&
                            __builtin_isfinite(cb.w) && __builtin_isfinite(sc);
        if (finite && cb.z - cb.x > 0.f && cb.w - cb.y > 0.f) cls = sc > cfg.obj_high ? 1 : (sc > cfg.obj_low ? 2 : 0);
        s.cbox[j] = cb;
        s.cscore[j] = sc;
        s.clabel[j] = labels[(int64_t)n * Q + j];
      }
      s.cls[j] = cls;
      s.out[j] = 0;
    }
    // 2. predict
    float mdx = 0.f, mdy = 0.f;
    bool moved = false;  // (uniform)
    if constexpr (kMotion == 1) {
      if (motion) {
        mdx = motion[4 * (int64_t)n], mdy = motion[4 * (int64_t)n + 1];
        moved = motion[4 * (int64_t)n + 2] == 1.0f && __builtin_isfinite(mdx) && __builtin_isfinite(mdy);
      }
    }
    float ma = 1.f, mb = 0.f, mpx = 0.f, mpy = 0.f, mqx = 0.f, mqy = 0.f, ms = 1.f;
    bool turned = false;  // (uniform)
    if constexpr (kMotion == 2) {
      if (motion) {
        const float* m = motion + 8 * (int64_t)n;
        mdx = m[0], mdy = m[1], ma = m[4], mb = m[5], mpx = m[6], mpy = m[7];
        const bool shift = __builtin_isfinite(mdx) && __builtin_isfinite(mdy);
        turned = m[3] == 2.0f && shift && __builtin_isfinite(ma) && __builtin_isfinite(mb) && __builtin_isfinite(mpx) &&
                 __builtin_isfinite(mpy);
        moved = m[3] == 1.0f && shift;
        mqx = mpx + mdx, mqy = mpy + mdy;
        ms = __builtin_sqrtf(ma * ma + mb * mb);  // (the correctly rounded sequence, not the bare v_sqrt_f32 of __fsqrt_rn)
      }
    }
    for (int t = tid; t < maxT; t += kThreads) {
      s.match[t] = -1;
      if (s.id[t] == 0) continue;
      if (s.last[t] != f - 1) s.mean[7 * maxT + t] = 0.f;
      const float h = s.mean[6 * maxT + t];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float* m = s.mean + (2 * c) * maxT + t;
        float* q = s.cov + (3 * c) * maxT + t;
        const float A = q[0], B = q[maxT], C = q[2 * maxT];
        const float sp = std_p(c, h), sv = std_v(c, h);
        m[0] = m[0] + m[maxT];
        q[0] = ((A + 2.f * B) + C) + sp * sp;
        q[maxT] = B + C;
        q[2 * maxT] = C + sv * sv;
      }
      if constexpr (kMotion != 0) {
        if (moved) s.mean[t] = s.mean[t] + mdx, s.mean[2 * maxT + t] = s.mean[2 * maxT + t] + mdy;
      }
      if constexpr (kMotion == 2) {
        if (turned) {
          const float ux = s.mean[t] - mpx, uy = s.mean[2 * maxT + t] - mpy;
          s.mean[t] = mqx + (ma * ux - mb * uy);
          s.mean[2 * maxT + t] = mqy + (mb * ux + ma * uy);
          const float vx = s.mean[maxT + t], vy = s.mean[3 * maxT + t];
          s.mean[maxT + t] = ma * vx - mb * vy;
          s.mean[3 * maxT + t] = mb * vx + ma * vy;
          s.mean[6 * maxT + t] = s.mean[6 * maxT + t] * ms;
          s.mean[7 * maxT + t] = s.mean[7 * maxT + t] * ms;
        }
      }
      const float cx = s.mean[t], cy = s.mean[2 * maxT + t], a = s.mean[4 * maxT + t], hh = s.mean[6 * maxT + t];
      const float w = a * hh;
      const float hw = w * 0.5f, hv = hh * 0.5f;
      s.tbox[t] = make_float4(cx - hw, cy - hv, cx + hw, cy + hv);
    }
    __syncthreads();
    if constexpr (kApp) {
      if (app.desc) app_addends(s, app, b, n, maxT, Q, cnt, f, lane, wave);  // (uniform; ends with a barrier)
    }

    // 3. to 5. the three associations
    associate(s, cnt, f);

    // 6. update the matched tracks, 7. free slots
    for (int t = tid; t < maxT; t += kThreads) {
      const int id = s.id[t];
      if (id == 0) continue;
      const int j = s.match[t];
      if (j >= 0) {
        const float4 cb = s.cbox[j];
        const float zh = cb.w - cb.y;
        const float z[4] = {(cb.x + cb.z) * 0.5f, (cb.y + cb.w) * 0.5f, (cb.z - cb.x) / zh, zh};
        const float h = s.mean[6 * maxT + t];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float* m = s.mean + (2 * c) * maxT + t;
          float* q = s.cov + (3 * c) * maxT + t;
          const float A = q[0], B = q[maxT], C = q[2 * maxT];
          const float sr = c == 2 ? 1e-1f : kWp * h;
          const float S = A + sr * sr;
          const float k0 = A / S, k1 = B / S;
          const float y = z[c] - m[0];
          m[0] = m[0] + k0 * y;
          m[maxT] = m[maxT] + k1 * y;
          q[0] = A - k0 * A;
          q[maxT] = B - k0 * B;
          q[2 * maxT] = C - k1 * B;
        }
        const int hits = s.hits[t] + 1;
        s.hits[t] = hits;
        s.last[t] = f;
        s.label[t] = s.clabel[j];
        int tent = s.tent[t];
        if (tent && hits >= cfg.tentatives) s.tent[t] = tent = 0;
        s.out[j] = tent ? -id : id;
      } else if (s.tent[t] != 0 || f - s.last[t] >= cfg.retain) {  // a freed slot is all zero
        s.id[t] = 0, s.hits[t] = 0, s.tent[t] = 0, s.last[t] = 0, s.label[t] = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) s.mean[i * maxT + t] = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) s.cov[i * maxT + t] = 0.f;
        if constexpr (kApp) s.match[t] = kAppFreed;
      }
    }
    __syncthreads();

    // 8. start tracks: the k-th starting candidate (ascending j) takes the k-th free slot (ascending)
    int nfree = 0;
    for (int base = 0; base < maxT; base += kThreads) {  // (uniform trip count)
      const int t = base + tid;
      const bool fr = t < maxT && s.id[t] == 0;
      int tot;
      const int r = nfree + block_rank(fr, s.wsum, lane, wave, tot);
      if (fr) s.freelist[r] = (unsigned short)t;
      nfree += tot;
    }
    __syncthreads();
    int nstart = 0;
    for (int base = 0; base < cnt; base += kThreads) {  // (uniform trip count)
      const int j = base + tid;
      const bool st = j < cnt && s.cls[j] == 1 && s.cscore[j] > cfg.init_thr;
      int tot;
      const int r = nstart + block_rank(st, s.wsum, lane, wave, tot);
      if (st && r < nfree) {
        const int t = s.freelist[r];
        const float4 cb = s.cbox[j];
        const float zh = cb.w - cb.y;
        const float z[4] = {(cb.x + cb.z) * 0.5f, (cb.y + cb.w) * 0.5f, (cb.z - cb.x) / zh, zh};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float sp = c == 2 ? 1e-2f : 2.f * std_p(c, zh), sv = c == 2 ? 1e-5f : 10.f * std_v(c, zh);
          s.mean[(2 * c) * maxT + t] = z[c];
          s.mean[(2 * c + 1) * maxT + t] = 0.f;
          s.cov[(3 * c) * maxT + t] = sp * sp;
          s.cov[(3 * c + 1) * maxT + t] = 0.f;
          s.cov[(3 * c + 2) * maxT + t] = sv * sv;
        }
        const int id = issued + r + 1, tent = f != 0;
        s.id[t] = id, s.hits[t] = 1, s.tent[t] = tent, s.last[t] = f, s.label[t] = s.clabel[j];
        s.out[j] = tent ? -id : id;
        if constexpr (kApp) s.match[t] = kAppStarted - j;
      }
      nstart += tot;
    }
    issued += min(nstart, nfree);
    refused += max(nstart - nfree, 0);
    __syncthreads();
    if constexpr (kApp) {
      if (app.desc) app_update(s, app, b, n, maxT, Q, cfg.obj_high, lane, wave);  // (uniform; ends with a barrier)
    }

    // 9. one id per candidate row, 0 beyond the count
    for (int j = tid; j < Q; j += kThreads) ids_out[(int64_t)n * Q + j] = j < cnt ? s.out[j] : 0;
    f += 1;
    __syncthreads();
  }

  if (tid == 0) s.hdr[0] = f, s.hdr[1] = issued, s.hdr[2] = refused, s.hdr[3] = 0;
  __syncthreads();
  {
    unsigned* g = reinterpret_cast<unsigned*>(states + (int64_t)b * sbytes);
    const unsigned* l = reinterpret_cast<const unsigned*>(lds_raw);
    for (int64_t i = tid; i < sbytes / 4; i += kThreads) g[i] = l[i];
  }
}

// the argument checks of codetr_track_update_* (all before any HIP call), then `launch(tab, cfg)` -> hipError_t
template <class Launch>
int checked_track_launch(const void* boxes, const void* scores, const int64_t* labels, const int* count, int64_t N,
                         int64_t Q, const int* stream_of_row, int64_t S, void* state, int64_t max_tracks,
                         const float* settings, int64_t retain, int64_t tentatives, int weight_iou, int* ids_out,
                         Launch launch) {
  if (!boxes || !scores || !labels || !count || !stream_of_row || !state || !settings || !ids_out || N <= 0 || Q <= 0 ||
      S <= 0 || max_tracks <= 0 || retain < 1 || tentatives < 1)
    return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX || Q > CODETR_POSTPROCESS_MAX_Q || max_tracks > CODETR_TRACK_MAX_TRACKS ||
      S > 0x7fffffffLL)
    return CODETR_E_TOO_LARGE;
  for (int i = 0; i < 6; ++i)
    if (!__builtin_isfinite(settings[i])) return CODETR_E_BADARG;
  RowTable tab = {};
  for (int64_t n = 0; n < N; ++n) {
    if (stream_of_row[n] < 0 || stream_of_row[n] >= S) return CODETR_E_BADARG;
    tab.stream[n] = stream_of_row[n];
  }
  for (int64_t n = N; n < CODETR_PREPROCESS_BATCH_MAX; ++n) tab.stream[n] = -1;
  const Settings cfg = {settings[0], settings[1], settings[2], settings[3], settings[4], settings[5],
                        (int)(retain > 0x7fffffffLL ? 0x7fffffffLL : retain),
                        (int)(tentatives > 0x7fffffffLL ? 0x7fffffffLL : tentatives), weight_iou ? 1 : 0};
  if (const hipError_t e = launch(tab, cfg); e != hipSuccess) return (int)e;
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace
