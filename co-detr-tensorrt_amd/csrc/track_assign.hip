// The tracker with a choice of association: codetr_track_update2_* of include/codetr_assign.h, and the same with the
// camera motion of every row added to the predicted centres: codetr_track_update3_* of include/codetr_motion.h, or applied as a
// similarity: codetr_track_update4_*, or with the appearance cue of include/codetr_appearance.h on top of that:
// codetr_track_update5_*.  The walk over a stream's
// frames, the filters, retirement and starts are track_common.h's (shared with track.hip and its pinned kernel); the
// greedy association is match_phase as it is there, the optimal one is assign_phase below, which hands the procedure of
// assign_core.h the integer gains of the header, computed on the fly from the boxes in LDS (no T x Q matrix).
//
// track_update2_kernel  one workgroup of 256 threads per stream, as track_update_kernel.  LDS: the tracker's + the
//                      solver's 8 T + 12 max(T, Q) + 96 bytes behind it: 114 KB at T = 512, Q = 1024.
//                      assign_phase: the phase's tracks with an eligible pair are found as the greedy phase finds its
//                      first bests (a wave per track, lanes over the candidates) and compacted in slot order into the
//                      free-slot list (unused until step 8); the columns are all candidates of the frame.
// fp32 with one rounding per operation: contraction is off for the whole file.
#pragma clang fp contract(off)
#include "track_common.h"

#include "assign_core.h"
#include "codetr_appearance.h"
#include "codetr_motion.h"

namespace {

static_assert(CODETR_TRACK_MAX_TRACKS <= CODETR_ASSIGN_MAX_ROWS && CODETR_POSTPROCESS_MAX_Q <= CODETR_ASSIGN_MAX_COLS,
              "the tracker's largest problem fits the solver");

__host__ __device__ inline int64_t lds2_offset(int64_t T, int64_t Q) { return round16(lds_bytes_of(T, Q)); }
__host__ __device__ inline int64_t lds2_bytes_of(int64_t T, int64_t Q) {
  return lds2_offset(T, Q) + assign_lds_bytes(T, T > Q ? T : Q);
}

// one optimal association (steps 3 to 5 of the rule under CODETR_ASSOCIATION_OPTIMAL); kind and cls as match_phase.
// Ends with a barrier.  kApp (codetr_appearance.h): `add` [T][pitch], the stream's appearance addends.
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
    const float iou = overlap(tb, box_area(tb), cb, box_area(cb));
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

template <class T>
__global__ __launch_bounds__(kThreads) void track_update2_kernel(const T* __restrict__ boxes, const T* __restrict__ scores,
                                                                 const int64_t* __restrict__ labels,
                                                                 const int* __restrict__ count, int N, int Q, RowTable tab,
                                                                 unsigned char* __restrict__ states, int maxT,
                                                                 Settings cfg, int* __restrict__ ids_out, int association) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const AssignLds a = assign_carve(lds_raw + lds2_offset(maxT, Q), maxT, max(maxT, Q));
  track_stream(lds_raw, boxes, scores, labels, count, N, Q, tab, states, maxT, cfg, ids_out,
               [&](const Lds& s, int cnt, int f) {  // 3. to 5. the three associations
                 const bool w = cfg.weight_iou != 0;
                 if (association == CODETR_ASSOCIATION_OPTIMAL) {  // (uniform)
                   assign_phase(s, a, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
                   assign_phase(s, a, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
                   assign_phase(s, a, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
                 } else {
                   match_phase(s, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
                   match_phase(s, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
                   match_phase(s, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
                 }
               });
}

// track_update2_kernel with the camera motion of every row (codetr_motion.h; `motion` [N, 4] or null) added to the predicted
// centres.  A kernel of its own, its text repeated, because the code of track_update2_kernel is pinned.
template <class T>
__global__ __launch_bounds__(kThreads) void track_update3_kernel(const T* __restrict__ boxes, const T* __restrict__ scores,
                                                                 const int64_t* __restrict__ labels,
                                                                 const int* __restrict__ count, int N, int Q, RowTable tab,
                                                                 unsigned char* __restrict__ states, int maxT,
                                                                 Settings cfg, int* __restrict__ ids_out, int association,
                                                                 const float* __restrict__ motion) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const AssignLds a = assign_carve(lds_raw + lds2_offset(maxT, Q), maxT, max(maxT, Q));
  track_stream<true>(
      lds_raw, boxes, scores, labels, count, N, Q, tab, states, maxT, cfg, ids_out,
      [&](const Lds& s, int cnt, int f) {  // 3. to 5. the three associations
        const bool w = cfg.weight_iou != 0;
        if (association == CODETR_ASSOCIATION_OPTIMAL) {  // (uniform)
          assign_phase(s, a, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
          assign_phase(s, a, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
          assign_phase(s, a, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
        } else {
          match_phase(s, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
          match_phase(s, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
          match_phase(s, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
        }
      },
      motion);
}

// track_update4_kernel with the similarity of every row (codetr_motion.h, version 2; `motion` [N, 8] or null): by the row's
// model the predicted centres, their velocities and the height are moved about (px, py), or the translation is added.
template <class T>
__global__ __launch_bounds__(kThreads) void track_update4_kernel(const T* __restrict__ boxes, const T* __restrict__ scores,
                                                                 const int64_t* __restrict__ labels,
                                                                 const int* __restrict__ count, int N, int Q, RowTable tab,
                                                                 unsigned char* __restrict__ states, int maxT,
                                                                 Settings cfg, int* __restrict__ ids_out, int association,
                                                                 const float* __restrict__ motion) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const AssignLds a = assign_carve(lds_raw + lds2_offset(maxT, Q), maxT, max(maxT, Q));
  track_stream<2>(
      lds_raw, boxes, scores, labels, count, N, Q, tab, states, maxT, cfg, ids_out,
      [&](const Lds& s, int cnt, int f) {  // 3. to 5. the three associations
        const bool w = cfg.weight_iou != 0;
        if (association == CODETR_ASSOCIATION_OPTIMAL) {  // (uniform)
          assign_phase(s, a, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
          assign_phase(s, a, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
          assign_phase(s, a, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
        } else {
          match_phase(s, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
          match_phase(s, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
          match_phase(s, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
        }
      },
      motion);
}

// track_update4_kernel with the appearance cue of codetr_appearance.h: `app.desc` [N, Q, 128] or null.  The first two
// associations take the pair values with the addends track_stream's pre-pass left in `app.add`; the third is as it was.
// With a null `app.desc` every branch below is update4's.  LDS as update2: the cue lives in global memory.
template <class T>
__global__ __launch_bounds__(kThreads) void track_update5_kernel(const T* __restrict__ boxes, const T* __restrict__ scores,
                                                                 const int64_t* __restrict__ labels,
                                                                 const int* __restrict__ count, int N, int Q, RowTable tab,
                                                                 unsigned char* __restrict__ states, int maxT,
                                                                 Settings cfg, int* __restrict__ ids_out, int association,
                                                                 const float* __restrict__ motion, App app) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const AssignLds a = assign_carve(lds_raw + lds2_offset(maxT, Q), maxT, max(maxT, Q));
  const float* add = app.desc ? app.add + (int64_t)blockIdx.x * maxT * Q : nullptr;
  track_stream<2, true>(
      lds_raw, boxes, scores, labels, count, N, Q, tab, states, maxT, cfg, ids_out,
      [&](const Lds& s, int cnt, int f) {  // 3. to 5. the three associations
        const bool w = cfg.weight_iou != 0;
        if (association == CODETR_ASSOCIATION_OPTIMAL) {  // (uniform)
          if (app.desc) {
            assign_phase<true>(s, a, maxT, cnt, f, 0, 1, w, cfg.match_high, tid, add, Q);
            assign_phase<true>(s, a, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid, add, Q);
          } else {
            assign_phase(s, a, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
            assign_phase(s, a, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
          }
          assign_phase(s, a, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
        } else {
          if (app.desc) {
            match_phase<true>(s, maxT, cnt, f, 0, 1, w, cfg.match_high, tid, add, Q);
            match_phase<true>(s, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid, add, Q);
          } else {
            match_phase(s, maxT, cnt, f, 0, 1, w, cfg.match_high, tid);
            match_phase(s, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid);
          }
          match_phase(s, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
        }
      },
      motion, app);
}

// the checks of codetr_track_update5_*'s own arguments (before any HIP call) -> 0 and `app`, or an error code
int app_of(const uint16_t* desc, void* app_state, const float* app_settings, void* work, int64_t work_bytes, int64_t S,
           int64_t max_tracks, int64_t Q, App& app) {
  app = App{};
  if (!desc) return 0;
  if (!app_state || !app_settings || !work || ((uintptr_t)desc & 15u) || ((uintptr_t)app_state & 3u) ||
      ((uintptr_t)work & 3u))
    return CODETR_E_BADARG;
  if (S <= 0 || max_tracks <= 0 || Q <= 0) return CODETR_E_BADARG;
  if (S > 0x7fffffffLL || max_tracks > CODETR_TRACK_MAX_TRACKS || Q > CODETR_POSTPROCESS_MAX_Q) return CODETR_E_TOO_LARGE;
  const float thr = app_settings[0], prox = app_settings[1], gate = app_settings[2];
  if (!__builtin_isfinite(thr) || !__builtin_isfinite(prox) || !__builtin_isfinite(gate) || thr < 0.f || thr > 1.f ||
      prox < 0.f || prox > 1.f || gate < 0.f)
    return CODETR_E_BADARG;
  if (work_bytes < 4 * S * max_tracks * Q) return CODETR_E_BADARG;
  app.desc = desc, app.g = static_cast<unsigned*>(app_state), app.add = static_cast<float*>(work);
  app.thr = thr, app.prox = prox, app.gate = gate;
  return 0;
}

template <class T>
int launch_track5(void* stream, const void* boxes, const void* scores, const int64_t* labels, const int* count, int64_t N,
                  int64_t Q, const int* stream_of_row, int64_t S, void* state, int64_t max_tracks, const float* settings,
                  int64_t retain, int64_t tentatives, int weight_iou, int* ids_out, int association, const float* motion,
                  const uint16_t* desc, void* app_state, const float* app_settings, void* work, int64_t work_bytes) {
  if (association != CODETR_ASSOCIATION_GREEDY && association != CODETR_ASSOCIATION_OPTIMAL) return CODETR_E_BADARG;
  App app;
  if (const int rc = app_of(desc, app_state, app_settings, work, work_bytes, S, max_tracks, Q, app)) return rc;
  return checked_track_launch(
      boxes, scores, labels, count, N, Q, stream_of_row, S, state, max_tracks, settings, retain, tentatives, weight_iou,
      ids_out, [&](const RowTable& tab, const Settings& cfg) -> hipError_t {
        const int64_t lds = lds2_bytes_of(max_tracks, Q);
        const int lds_max = (int)lds2_bytes_of(CODETR_TRACK_MAX_TRACKS, CODETR_POSTPROCESS_MAX_Q);
        if (lds + kStaticLds > 64 * 1024)
          if (const hipError_t e = allow_large_lds<track_update5_kernel<T>>(lds_max); e != hipSuccess) return e;
        hipLaunchKernelGGL((track_update5_kernel<T>), dim3((unsigned)S), dim3(kThreads), (size_t)lds,
                           static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                           labels, count, (int)N, (int)Q, tab, static_cast<unsigned char*>(state), (int)max_tracks, cfg,
                           ids_out, association, motion, app);
        return hipSuccess;
      });
}

template <class T, int kMotion = 0>
int launch_track2(void* stream, const void* boxes, const void* scores, const int64_t* labels, const int* count, int64_t N,
                  int64_t Q, const int* stream_of_row, int64_t S, void* state, int64_t max_tracks, const float* settings,
                  int64_t retain, int64_t tentatives, int weight_iou, int* ids_out, int association,
                  const float* motion = nullptr) {
  if (association != CODETR_ASSOCIATION_GREEDY && association != CODETR_ASSOCIATION_OPTIMAL) return CODETR_E_BADARG;
  return checked_track_launch(
      boxes, scores, labels, count, N, Q, stream_of_row, S, state, max_tracks, settings, retain, tentatives, weight_iou,
      ids_out, [&](const RowTable& tab, const Settings& cfg) -> hipError_t {
        const int64_t lds = lds2_bytes_of(max_tracks, Q);
        const int lds_max = (int)lds2_bytes_of(CODETR_TRACK_MAX_TRACKS, CODETR_POSTPROCESS_MAX_Q);
        if constexpr (kMotion == 2) {
          if (lds + kStaticLds > 64 * 1024)
            if (const hipError_t e = allow_large_lds<track_update4_kernel<T>>(lds_max); e != hipSuccess) return e;
          hipLaunchKernelGGL((track_update4_kernel<T>), dim3((unsigned)S), dim3(kThreads), (size_t)lds,
                             static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                             labels, count, (int)N, (int)Q, tab, static_cast<unsigned char*>(state), (int)max_tracks, cfg,
                             ids_out, association, motion);
        } else if constexpr (kMotion == 1) {
          if (lds + kStaticLds > 64 * 1024)  // (the opt-in is needed once dynamic + static LDS pass 64 KB)
            if (const hipError_t e = allow_large_lds<track_update3_kernel<T>>(lds_max); e != hipSuccess) return e;
          hipLaunchKernelGGL((track_update3_kernel<T>), dim3((unsigned)S), dim3(kThreads), (size_t)lds,
                             static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                             labels, count, (int)N, (int)Q, tab, static_cast<unsigned char*>(state), (int)max_tracks, cfg,
                             ids_out, association, motion);
        } else {
          if (lds + kStaticLds > 64 * 1024)
            if (const hipError_t e = allow_large_lds<track_update2_kernel<T>>(lds_max); e != hipSuccess) return e;
          hipLaunchKernelGGL((track_update2_kernel<T>), dim3((unsigned)S), dim3(kThreads), (size_t)lds,
                             static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                             labels, count, (int)N, (int)Q, tab, static_cast<unsigned char*>(state), (int)max_tracks, cfg,
                             ids_out, association);
        }
        return hipSuccess;
      });
}

}  // namespace

extern "C" {

#define CODETR_TRACK2_ENTRY(SUFFIX, TYPE)                                                                                  \
  int codetr_track_update2_##SUFFIX(void* stream, const void* boxes_dev, const void* scores_dev,                           \
                                    const int64_t* labels_dev, const int* count_dev, int64_t N, int64_t Q,                 \
                                    const int* stream_of_row_host, int64_t S, void* state_dev, int64_t max_tracks,         \
                                    const float* settings_host, int64_t retain, int64_t tentatives, int weight_iou,        \
                                    int* track_id_out_dev, int association) {                                              \
    return launch_track2<TYPE>(stream, boxes_dev, scores_dev, labels_dev, count_dev, N, Q, stream_of_row_host, S,          \
                               state_dev, max_tracks, settings_host, retain, tentatives, weight_iou, track_id_out_dev,     \
                               association);                                                                               \
  }
CODETR_TRACK2_ENTRY(f16, _Float16)
CODETR_TRACK2_ENTRY(bf16, Bf16)
CODETR_TRACK2_ENTRY(f32, float)
#undef CODETR_TRACK2_ENTRY

#define CODETR_TRACK3_ENTRY(SUFFIX, TYPE)                                                                                  \
  int codetr_track_update3_##SUFFIX(void* stream, const void* boxes_dev, const void* scores_dev,                           \
                                    const int64_t* labels_dev, const int* count_dev, int64_t N, int64_t Q,                 \
                                    const int* stream_of_row_host, int64_t S, void* state_dev, int64_t max_tracks,         \
                                    const float* settings_host, int64_t retain, int64_t tentatives, int weight_iou,        \
                                    int* track_id_out_dev, int association, const float* motion_dev) {                     \
    return launch_track2<TYPE, 1>(stream, boxes_dev, scores_dev, labels_dev, count_dev, N, Q, stream_of_row_host, S,    \
                                     state_dev, max_tracks, settings_host, retain, tentatives, weight_iou,                 \
                                     track_id_out_dev, association, motion_dev);                                           \
  }
CODETR_TRACK3_ENTRY(f16, _Float16)
CODETR_TRACK3_ENTRY(bf16, Bf16)
CODETR_TRACK3_ENTRY(f32, float)
#undef CODETR_TRACK3_ENTRY

#define CODETR_TRACK4_ENTRY(SUFFIX, TYPE)                                                                                  \
  int codetr_track_update4_##SUFFIX(void* stream, const void* boxes_dev, const void* scores_dev,                           \
                                    const int64_t* labels_dev, const int* count_dev, int64_t N, int64_t Q,                 \
                                    const int* stream_of_row_host, int64_t S, void* state_dev, int64_t max_tracks,         \
                                    const float* settings_host, int64_t retain, int64_t tentatives, int weight_iou,        \
                                    int* track_id_out_dev, int association, const float* motion_dev) {                     \
    return launch_track2<TYPE, 2>(stream, boxes_dev, scores_dev, labels_dev, count_dev, N, Q, stream_of_row_host, S,       \
                                  state_dev, max_tracks, settings_host, retain, tentatives, weight_iou, track_id_out_dev,  \
                                  association, motion_dev);                                                                \
  }
CODETR_TRACK4_ENTRY(f16, _Float16)
CODETR_TRACK4_ENTRY(bf16, Bf16)
CODETR_TRACK4_ENTRY(f32, float)
#undef CODETR_TRACK4_ENTRY

#define CODETR_TRACK5_ENTRY(SUFFIX, TYPE)                                                                                  \
  int codetr_track_update5_##SUFFIX(void* stream, const void* boxes_dev, const void* scores_dev,                           \
                                    const int64_t* labels_dev, const int* count_dev, int64_t N, int64_t Q,                 \
                                    const int* stream_of_row_host, int64_t S, void* state_dev, int64_t max_tracks,         \
                                    const float* settings_host, int64_t retain, int64_t tentatives, int weight_iou,        \
                                    int* track_id_out_dev, int association, const float* motion_dev,                       \
                                    const uint16_t* desc_dev, void* app_state_dev, const float* app_settings_host,         \
                                    void* work_dev, int64_t work_bytes) {                                                  \
    return launch_track5<TYPE>(stream, boxes_dev, scores_dev, labels_dev, count_dev, N, Q, stream_of_row_host, S,          \
                               state_dev, max_tracks, settings_host, retain, tentatives, weight_iou, track_id_out_dev,     \
                               association, motion_dev, desc_dev, app_state_dev, app_settings_host, work_dev, work_bytes); \
  }
CODETR_TRACK5_ENTRY(f16, _Float16)
CODETR_TRACK5_ENTRY(bf16, Bf16)
CODETR_TRACK5_ENTRY(f32, float)
#undef CODETR_TRACK5_ENTRY

}  // extern "C"
