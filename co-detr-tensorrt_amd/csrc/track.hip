// The Inferencer's tracking-by-detection on the GPU: a chunk's final detections (whatever post-processing or merge launch
// produced them) -> one track id per detection row, the streams' track states kept on the device between calls.  The rule
// -- candidates, the four two-state Kalman filters, the three associations, retirement and track starts -- is stated
// operation by operation in include/codetr_hip.h ("Tracking"); the companion headers add the choice of association
// (codetr_assign.h), the camera motion of every row (codetr_motion.h) and the appearance cue (codetr_appearance.h).
// This file holds the kernel, its launcher and the entry points; the device code they instantiate is track_common.h's.
//
// track_kernel  ONE kernel text for every form of the update; a form is an instantiation and an entry point:
//                 codetr_track_update_*   <false, 0, false, T>                                    greedy only
//                 codetr_track_update2_*  <true, 0, false, T, int>                                + association
//                 codetr_track_update3_*  <true, 1, false, T, int, const float* __restrict__>     + motion [N, 4]
//                 codetr_track_update4_*  <true, 2, false, T, int, const float* __restrict__>     + motion [N, 8]
//                 codetr_track_update5_*  <true, 2, true, T, int, const float* __restrict__, App> + the appearance cue
//               The trailing pack is the form's own kernel arguments, so every form keeps the argument layout and the
//               machine code it had as a kernel of its own (tools/isa_extract.py diff --pair; profiles/r28_track_unify.txt).
//               A NEW FORM IS A NEW INSTANTIATION AND A NEW ENTRY, not a new kernel text.
//               One workgroup of 256 threads per stream.  The stream's rows of the launch are walked in row order inside the
//               one launch (a chunk of 8 frames of one camera is one launch); the state is read from the caller's buffer
//               into LDS once and written back once, a stream without a row is not touched.  LDS: the state as laid out
//               in the header (16 + 104 T bytes) + 24 T bytes of working arrays + 33 bytes per candidate row: 98 KB at
//               T = 512, Q = 1024 (under 64 KB up to T = 256 with Q = 1024); kSolver adds the solver's behind it.
//               Greedy association without a T x Q matrix: every thread owns the tracks tid and tid + 256 and keeps
//               their best free candidate (value, lowest j) in registers; a best is (re)computed by the owner's wave
//               together -- lanes stride over the candidates, one wave arg-max.  A pick is one workgroup arg-max (value,
//               then lowest slot; one barrier, double-buffered partials); then only the tracks whose best was the
//               candidate just taken are recomputed.  Track starts take the k-th free slot for the k-th starting
//               candidate through two workgroup scans.
// fp32 with one rounding per operation: contraction is off for the whole file, divisions are IEEE.
// A separate translation unit from prepost.hip on purpose: the code of the kernels there is pinned.
#pragma clang fp contract(off)
#include "track_common.h"

#include <type_traits>

namespace {

// a form's trailing kernel arguments (none, or the first one, two or three of these) with the defaults of the rest
struct Extras {
  int association;
  const float* __restrict__ motion;
  App app;
};
__host__ __device__ __forceinline__ Extras extras_of(int association = CODETR_ASSOCIATION_GREEDY,
                                                     const float* __restrict__ motion = nullptr, App app = {}) {
  return {association, motion, app};
}

// kSolver: the form has an `association` and carves the solver's LDS; kMotion, kApp: track_stream's.  At an instantiation
// the motion pointer of the pack is spelled `const float* __restrict__`: deduced from a call it would lose the qualifier.
template <bool kSolver, int kMotion, bool kApp, class T, class... X>
__global__ __launch_bounds__(kThreads) void track_kernel(const T* __restrict__ boxes, const T* __restrict__ scores,
                                                         const int64_t* __restrict__ labels,
                                                         const int* __restrict__ count, int N, int Q, RowTable tab,
                                                         unsigned char* __restrict__ states, int maxT, Settings cfg,
                                                         int* __restrict__ ids_out, X... x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const Extras e = extras_of(x...);
  AssignLds a = {};
  if constexpr (kSolver) a = assign_carve(lds_raw + lds2_offset(maxT, Q), maxT, max(maxT, Q));
  const float* add = nullptr;  // the stream's appearance addends, when the cue is on
  if constexpr (kApp) add = e.app.desc ? e.app.add + (int64_t)blockIdx.x * maxT * Q : nullptr;
  track_stream<kMotion, kApp>(
      lds_raw, boxes, scores, labels, count, N, Q, tab, states, maxT, cfg, ids_out,
      [&](const Lds& s, int cnt, int f) {  // 3. to 5. the three associations: the first two with the cue or without
        const bool w = cfg.weight_iou != 0;
        const auto with_cue_or_not = [&](auto first_two) {
          if constexpr (kApp) {
            if (e.app.desc) return first_two(std::true_type{});  // (uniform)
          }
          first_two(std::false_type{});
        };
        if constexpr (kSolver) {
          if (e.association == CODETR_ASSOCIATION_OPTIMAL) {  // (uniform)
            with_cue_or_not([&](auto cue) {
              assign_phase<decltype(cue)::value>(s, a, maxT, cnt, f, 0, 1, w, cfg.match_high, tid, add, Q);
              assign_phase<decltype(cue)::value>(s, a, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid, add, Q);
            });
            assign_phase(s, a, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
            return;
          }
        }
        with_cue_or_not([&](auto cue) {
          match_phase<decltype(cue)::value>(s, maxT, cnt, f, 0, 1, w, cfg.match_high, tid, add, Q);
          match_phase<decltype(cue)::value>(s, maxT, cnt, f, 1, 1, w, cfg.match_tentative, tid, add, Q);
        });
        match_phase(s, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
      },
      e.motion, e.app);
}

// the argument checks in the order every form has had them -- `association` (kSolver), the cue's own (app_of, by the
// entry), then checked_track_launch's -- and the one launch.  x: the kernel's trailing arguments, their types named.
template <bool kSolver, int kMotion, bool kApp, class T, class... X>
int launch_track(void* stream, const void* boxes, const void* scores, const int64_t* labels, const int* count, int64_t N,
                 int64_t Q, const int* stream_of_row, int64_t S, void* state, int64_t max_tracks, const float* settings,
                 int64_t retain, int64_t tentatives, int weight_iou, int* ids_out, X... x) {
  if constexpr (kSolver) {
    const int association = extras_of(x...).association;
    if (association != CODETR_ASSOCIATION_GREEDY && association != CODETR_ASSOCIATION_OPTIMAL) return CODETR_E_BADARG;
  }
  return checked_track_launch(
      boxes, scores, labels, count, N, Q, stream_of_row, S, state, max_tracks, settings, retain, tentatives, weight_iou,
      ids_out, [&](const RowTable& tab, const Settings& cfg) -> hipError_t {
        constexpr auto kernel = track_kernel<kSolver, kMotion, kApp, T, X...>;
        constexpr auto bytes_of = kSolver ? lds2_bytes_of : lds_bytes_of;
        const int64_t lds = bytes_of(max_tracks, Q);
        if (lds + kStaticLds > 64 * 1024)  // (the opt-in is needed once dynamic + static LDS pass 64 KB)
          if (const hipError_t err = allow_large_lds<kernel>(
                  (int)bytes_of(CODETR_TRACK_MAX_TRACKS, CODETR_POSTPROCESS_MAX_Q));
              err != hipSuccess)
            return err;
        hipLaunchKernelGGL(kernel, dim3((unsigned)S), dim3(kThreads), (size_t)lds, static_cast<hipStream_t>(stream),
                           static_cast<const T*>(boxes), static_cast<const T*>(scores), labels, count, (int)N, (int)Q, tab,
                           static_cast<unsigned char*>(state), (int)max_tracks, cfg, ids_out, x...);
        return hipSuccess;
      });
}

// the forms (the table of the file's head): a new one is one more line here and one more TRACK_ENTRIES below
template <class T>
constexpr auto track1 = launch_track<false, 0, false, T>;
template <class T>
constexpr auto track2 = launch_track<true, 0, false, T, int>;
template <class T>
constexpr auto track3 = launch_track<true, 1, false, T, int, const float* __restrict__>;
template <class T>
constexpr auto track4 = launch_track<true, 2, false, T, int, const float* __restrict__>;
template <class T>
constexpr auto track5 = launch_track<true, 2, true, T, int, const float* __restrict__, App>;

// the checks of codetr_track_update5_*'s own arguments (before any HIP call) -> 0 and `app`, or an error code.  The
// association comes first in the entry's order of checks, so it is looked at here too.
int app_of(int association, const uint16_t* desc, void* app_state, const float* app_settings, void* work,
           int64_t work_bytes, int64_t S, int64_t max_tracks, int64_t Q, App& app) {
  app = App{};
  if (association != CODETR_ASSOCIATION_GREEDY && association != CODETR_ASSOCIATION_OPTIMAL) return CODETR_E_BADARG;
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

}  // namespace

extern "C" {

int64_t codetr_track_state_bytes(int64_t max_tracks) {
  if (max_tracks <= 0 || max_tracks > CODETR_TRACK_MAX_TRACKS) return CODETR_E_BADARG;
  return state_bytes_of(max_tracks);
}

// codetr_track_update<FORM>_<f16 | bf16 | f32>(PARAMS) { BODY }, T the element type in BODY
#define TRACK_PARAMS                                                                                                     \
  void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev, const int *count_dev, int64_t N, \
      int64_t Q, const int *stream_of_row_host, int64_t S, void *state_dev, int64_t max_tracks,                          \
      const float *settings_host, int64_t retain, int64_t tentatives, int weight_iou, int *track_id_out_dev
#define TRACK_ARGS                                                                                                   \
  stream, boxes_dev, scores_dev, labels_dev, count_dev, N, Q, stream_of_row_host, S, state_dev, max_tracks, settings_host, \
      retain, tentatives, weight_iou, track_id_out_dev
#define TRACK_ENTRY(FORM, SUFFIX, TYPE, PARAMS, BODY) \
  int codetr_track_update##FORM##_##SUFFIX PARAMS {   \
    using T = TYPE;                                   \
    BODY                                              \
  }
#define TRACK_ENTRIES(FORM, PARAMS, BODY)         \
  TRACK_ENTRY(FORM, f16, _Float16, PARAMS, BODY)  \
  TRACK_ENTRY(FORM, bf16, Bf16, PARAMS, BODY)     \
  TRACK_ENTRY(FORM, f32, float, PARAMS, BODY)

TRACK_ENTRIES(, (TRACK_PARAMS), return track1<T>(TRACK_ARGS);)
TRACK_ENTRIES(2, (TRACK_PARAMS, int association), return track2<T>(TRACK_ARGS, association);)
TRACK_ENTRIES(3, (TRACK_PARAMS, int association, const float* motion_dev),
              return track3<T>(TRACK_ARGS, association, motion_dev);)
TRACK_ENTRIES(4, (TRACK_PARAMS, int association, const float* motion_dev),
              return track4<T>(TRACK_ARGS, association, motion_dev);)
TRACK_ENTRIES(5,
              (TRACK_PARAMS, int association, const float* motion_dev, const uint16_t* desc_dev, void* app_state_dev,
               const float* app_settings_host, void* work_dev, int64_t work_bytes),
              App app;
              if (const int rc = app_of(association, desc_dev, app_state_dev, app_settings_host, work_dev, work_bytes, S,
                                        max_tracks, Q, app)) return rc;
              return track5<T>(TRACK_ARGS, association, motion_dev, app);)

#undef TRACK_ENTRIES
#undef TRACK_ENTRY
#undef TRACK_ARGS
#undef TRACK_PARAMS

}  // extern "C"
