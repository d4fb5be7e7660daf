// The assignment procedure of include/codetr_assign.h as device code for one workgroup of 256 threads, written once:
// assign.hip (codetr_assign_i32) gives it gains read from memory, the tracker (track_common.h) gains computed on the fly
// from the boxes in LDS.  Integer arithmetic only; every loop is counted.
//
// A thread owns the columns tid, tid + 256, .. (at most kAsgOwn): their dist and visited flags live in its registers.
// u, v, pred and owner are in LDS (assign_lds_bytes).  A round = one relax of the thread's columns against the current
// row, one workgroup arg-min (least dist, ties to the lowest column: wave shuffles, then kAsgWaves partials that are
// double-buffered, so one barrier per round suffices), and the bookkeeping every thread repeats on the uniform result.
// The duals are updated once per augmentation from the final distance (the header shows it equals a per-round update).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_assign.h"

namespace {

constexpr int kAsgThreads = 256;
constexpr int kAsgWaves = kAsgThreads / 64;
constexpr int kAsgOwn = CODETR_ASSIGN_MAX_COLS / kAsgThreads;  // columns a thread owns
constexpr int kAsgNone = 0x7fffffff;
constexpr long long kAsgInf = 1LL << 62;
static_assert(CODETR_ASSIGN_MAX_COLS % kAsgThreads == 0, "a whole number of columns per thread");
static_assert(CODETR_ASSIGN_MAX_ROWS <= CODETR_ASSIGN_MAX_COLS && CODETR_ASSIGN_MAX_COLS <= 32767,
              "owner and pred are 16-bit");

struct AssignLds {
  long long* u;      // [R]
  long long* v;      // [M]
  long long* red_d;  // [2][kAsgWaves]
  int* red_j;        // [2][kAsgWaves]
  short* pred;       // [M] the column through which a column was reached, -1: from the start
  short* owner;      // [M] the row that holds a column, -1: free
};

// R: rows, M: columns (virtual ones included), as the carve is given them
__host__ __device__ constexpr int64_t assign_lds_bytes(int64_t R, int64_t M) {
  return (8 * R + 8 * M + 24 * kAsgWaves + 4 * M + 15) / 16 * 16;
}

// base: 8-byte aligned
__device__ __forceinline__ AssignLds assign_carve(unsigned char* base, int R, int M) {
  AssignLds a;
  unsigned char* p = base;
  a.u = (long long*)p, p += 8 * R;
  a.v = (long long*)p, p += 8 * M;
  a.red_d = (long long*)p, p += 16 * kAsgWaves;
  a.red_j = (int*)p, p += 8 * kAsgWaves;
  a.pred = (short*)p, p += 2 * M;
  a.owner = (short*)p;
  return a;
}

// R <= CODETR_ASSIGN_MAX_ROWS rows against M <= CODETR_ASSIGN_MAX_COLS columns, R <= M; gain(i, j) in
// [0, CODETR_ASSIGN_MAX_GAIN] for every (i, j), virtual columns included (the caller's functor answers 0 there), and the
// same value whenever it is asked.  All arguments are workgroup-uniform.  On return a.owner[j] is the row of column j or
// -1; ends with a barrier.
template <class Gain>
__device__ __forceinline__ void assign_solve(const AssignLds& a, int R, int M, Gain gain, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < M; j += kAsgThreads) a.v[j] = 0, a.owner[j] = -1;
  for (int i = tid; i < R; i += kAsgThreads) a.u[i] = 0;
  __syncthreads();
  int buf = 0;
  for (int i = 0; i < R; ++i) {  // one augmentation per row, in ascending order
    long long dist[kAsgOwn];
    bool vis[kAsgOwn];
#pragma unroll
    for (int k = 0; k < kAsgOwn; ++k) dist[k] = kAsgInf, vis[k] = false;
    int r = i, through = -1, sink = -1;
    long long D = 0;
    for (int round = 0; round <= M; ++round) {  // (a search ends within M rounds: one more column is visited in each)
      const long long ur = a.u[r];
      long long bd = kAsgInf;
      int bj = kAsgNone;
#pragma unroll
      for (int k = 0; k < kAsgOwn; ++k) {  // (ascending j: a tie keeps the lower)
        const int j = tid + k * kAsgThreads;
        if (j < M && !vis[k]) {
          const long long d = D - (long long)gain(r, j) - ur - a.v[j];
          if (d < dist[k]) dist[k] = d, a.pred[j] = (short)through;
          if (dist[k] < bd) bd = dist[k], bj = j;
        }
      }
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        const long long od = __shfl_xor(bd, m, 64);
        const int oj = __shfl_xor(bj, m, 64);
        if (oj != kAsgNone && (bj == kAsgNone || od < bd || (od == bd && oj < bj))) bd = od, bj = oj;
      }
      if (lane == 0) a.red_d[buf * kAsgWaves + wave] = bd, a.red_j[buf * kAsgWaves + wave] = bj;
      __syncthreads();
      bd = kAsgInf, bj = kAsgNone;
#pragma unroll
      for (int w = 0; w < kAsgWaves; ++w) {
        const long long od = a.red_d[buf * kAsgWaves + w];
        const int oj = a.red_j[buf * kAsgWaves + w];
        if (oj != kAsgNone && (bj == kAsgNone || od < bd || (od == bd && oj < bj))) bd = od, bj = oj;
      }
      buf ^= 1;
      if (bj == kAsgNone) break;  // (uniform; every column visited: cannot happen while R <= M)
      D = bd;
#pragma unroll
      for (int k = 0; k < kAsgOwn; ++k)
        if (bj == tid + k * kAsgThreads) vis[k] = true;
      const int o = a.owner[bj];  // (owner is only written between searches)
      if (o < 0) {
        sink = bj;
        break;
      }
      r = o, through = bj;
    }
    if (sink >= 0) {  // (uniform)
#pragma unroll
      for (int k = 0; k < kAsgOwn; ++k)
        if (vis[k]) {  // (the owners of the visited columns are distinct rows, none of them i)
          const int j = tid + k * kAsgThreads;
          const long long d = D - dist[k];
          a.v[j] -= d;
          const int o = a.owner[j];
          if (o >= 0) a.u[o] += d;
        }
      if (tid == 0) a.u[i] += D;
    }
    __syncthreads();
    if (tid == 0 && sink >= 0) {
      int j = sink;
      for (int step = 0; step <= M && j >= 0; ++step) {  // (a path holds every column at most once)
        const int p = a.pred[j];
        a.owner[j] = p < 0 ? (short)i : a.owner[p];
        j = p;
      }
    }
    __syncthreads();
  }
}

}  // namespace
