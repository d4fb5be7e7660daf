// The Inferencer's tracking-by-detection on the GPU: a chunk's final detections (whatever post-processing or merge launch
// produced them) -> one track id per detection row, the streams' track states kept on the device between calls.  The rule
// -- candidates, the four two-state Kalman filters, the three greedy associations, retirement and track starts -- is
// stated operation by operation in include/codetr_hip.h ("Tracking"); this file and track_common.h follow that text.
//
// track_update_kernel  one workgroup of 256 threads per stream.  The stream's rows of the launch are walked in row order
//                     inside the one launch (a chunk of 8 frames of one camera is one launch); the state is read from the
//                     caller's buffer into LDS once and written back once, a stream without a row is not touched.  LDS:
//                     the state as laid out in the header (16 + 104 T bytes) + 24 T bytes of working arrays + 33 bytes
//                     per candidate row: 98 KB at T = 512, Q = 1024 (under 64 KB up to T = 256 with Q = 1024).
//                     Greedy association without a T x Q matrix: every thread owns the tracks tid and tid + 256 and keeps
//                     their best free candidate (value, lowest j) in registers; a best is (re)computed by the owner's
//                     wave together -- lanes stride over the candidates, one wave arg-max.  A pick is one workgroup
//                     arg-max (value, then lowest slot; one barrier, double-buffered partials); then only the tracks
//                     whose best was the candidate just taken are recomputed.  Track starts take the k-th free slot for
//                     the k-th starting candidate through two workgroup scans.
// fp32 with one rounding per operation: contraction is off for the whole file, divisions are IEEE.
// A separate translation unit from prepost.hip on purpose: the code of the kernels there is pinned.  The body lives in
// track_common.h, which track_assign.hip (codetr_track_update2_*: the same walk with a choice of association) shares.
#pragma clang fp contract(off)
#include "track_common.h"

namespace {

template <class T>
__global__ __launch_bounds__(kThreads) void track_update_kernel(const T* __restrict__ boxes, const T* __restrict__ scores,
                                                                const int64_t* __restrict__ labels,
                                                                const int* __restrict__ count, int N, int Q, RowTable tab,
                                                                unsigned char* __restrict__ states, int maxT, Settings cfg,
                                                                int* __restrict__ ids_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  track_stream(lds_raw, boxes, scores, labels, count, N, Q, tab, states, maxT, cfg, ids_out,
               [&](const Lds& s, int cnt, int f) {  // 3. to 5. the three associations
                 match_phase(s, maxT, cnt, f, 0, 1, cfg.weight_iou != 0, cfg.match_high, tid);
                 match_phase(s, maxT, cnt, f, 1, 1, cfg.weight_iou != 0, cfg.match_tentative, tid);
                 match_phase(s, maxT, cnt, f, 2, 2, false, cfg.match_low, tid);
               });
}

template <class T>
int launch_track(void* stream, const void* boxes, const void* scores, const int64_t* labels, const int* count, int64_t N,
                 int64_t Q, const int* stream_of_row, int64_t S, void* state, int64_t max_tracks, const float* settings,
                 int64_t retain, int64_t tentatives, int weight_iou, int* ids_out) {
  return checked_track_launch(
      boxes, scores, labels, count, N, Q, stream_of_row, S, state, max_tracks, settings, retain, tentatives, weight_iou,
      ids_out, [&](const RowTable& tab, const Settings& cfg) -> hipError_t {
        const int64_t lds = lds_bytes_of(max_tracks, Q);
        if (lds + kStaticLds > 64 * 1024)  // (the opt-in is needed once dynamic + static LDS pass 64 KB)
          if (const hipError_t e = allow_large_lds<track_update_kernel<T>>(
                  (int)lds_bytes_of(CODETR_TRACK_MAX_TRACKS, CODETR_POSTPROCESS_MAX_Q));
              e != hipSuccess)
            return e;
        hipLaunchKernelGGL((track_update_kernel<T>), dim3((unsigned)S), dim3(kThreads), (size_t)lds,
                           static_cast<hipStream_t>(stream), static_cast<const T*>(boxes), static_cast<const T*>(scores),
                           labels, count, (int)N, (int)Q, tab, static_cast<unsigned char*>(state), (int)max_tracks, cfg,
                           ids_out);
        return hipSuccess;
      });
}

}  // namespace

extern "C" {

int64_t codetr_track_state_bytes(int64_t max_tracks) {
  if (max_tracks <= 0 || max_tracks > CODETR_TRACK_MAX_TRACKS) return CODETR_E_BADARG;
  return state_bytes_of(max_tracks);
}

#define CODETR_TRACK_ENTRY(SUFFIX, TYPE)                                                                                  \
  int codetr_track_update_##SUFFIX(void* stream, const void* boxes_dev, const void* scores_dev, const int64_t* labels_dev, \
                                   const int* count_dev, int64_t N, int64_t Q, const int* stream_of_row_host, int64_t S,  \
                                   void* state_dev, int64_t max_tracks, const float* settings_host, int64_t retain,       \
                                   int64_t tentatives, int weight_iou, int* track_id_out_dev) {                           \
    return launch_track<TYPE>(stream, boxes_dev, scores_dev, labels_dev, count_dev, N, Q, stream_of_row_host, S,          \
                              state_dev, max_tracks, settings_host, retain, tentatives, weight_iou, track_id_out_dev);    \
  }
CODETR_TRACK_ENTRY(f16, _Float16)
CODETR_TRACK_ENTRY(bf16, Bf16)
CODETR_TRACK_ENTRY(f32, float)
#undef CODETR_TRACK_ENTRY

}  // extern "C"
