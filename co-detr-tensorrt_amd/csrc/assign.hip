// Linear assignment on the GPU: codetr_assign_i32 of include/codetr_assign.h, one workgroup per problem.  The procedure
// -- shortest augmenting paths over integer costs with a stated tie rule -- is written once in assign_core.h; this file
// gives it gains read from memory (clamped as the header says) and writes the matches and their total.
//
// assign_kernel  256 threads per problem, 16.1 KB of static LDS.  A round reads one row of the gain matrix, coalesced
//                (a thread its columns tid, tid + 256, ..).  Afterwards owner[] is turned into the row-wise result through
//                LDS (the u array is free by then), so that every element of match_out is written exactly once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assign_core.h"
#include "codetr_hip.h"

namespace {

__global__ __launch_bounds__(kAsgThreads) void assign_kernel(const int* __restrict__ gain, int n, int m,
                                                             int* __restrict__ match_out,
                                                             long long* __restrict__ total_out) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[assign_lds_bytes(CODETR_ASSIGN_MAX_ROWS, CODETR_ASSIGN_MAX_COLS)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int* g = gain + b * n * m;
  const int M = max(n, m);
  const AssignLds a = assign_carve(raw, n, M);
  const auto gain_of = [&](int i, int j) -> int {
    return j < m ? min(max(g[(int64_t)i * m + j], 0), CODETR_ASSIGN_MAX_GAIN) : 0;  // (virtual columns: 0)
  };
  assign_solve(a, n, M, gain_of, tid);

  int* row_match = reinterpret_cast<int*>(a.u);  // (the duals are done with)
  for (int i = tid; i < n; i += kAsgThreads) row_match[i] = -1;
  __syncthreads();
  long long sum = 0;
  for (int j = tid; j < m; j += kAsgThreads) {
    const int o = a.owner[j];
    if (o < 0) continue;
    const int v = gain_of(o, j);
    if (v > 0) row_match[o] = j, sum += v;  // (a pair of gain 0 is not reported)
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
  if (lane == 0) a.red_d[wave] = sum;
  __syncthreads();
  for (int i = tid; i < n; i += kAsgThreads) match_out[b * n + i] = row_match[i];
  if (tid == 0) {
    long long t = 0;
    for (int w = 0; w < kAsgWaves; ++w) t += a.red_d[w];
    total_out[b] = t;
  }
}

}  // namespace

extern "C" {

int codetr_assign_abi_version(void) { return CODETR_ASSIGN_ABI_VERSION; }

int codetr_assign_i32(void* stream, const int* gain_dev, int64_t B, int64_t n, int64_t m, int* match_out_dev,
                      int64_t* total_out_dev) {
  if (!gain_dev || !match_out_dev || !total_out_dev || B <= 0 || n <= 0 || m <= 0) return CODETR_E_BADARG;
  if (n > CODETR_ASSIGN_MAX_ROWS || m > CODETR_ASSIGN_MAX_COLS || B > 65535) return CODETR_E_TOO_LARGE;
  static_assert(sizeof(long long) == sizeof(int64_t), "total_out is written as long long");
  hipLaunchKernelGGL(assign_kernel, dim3((unsigned)B), dim3(kAsgThreads), 0, static_cast<hipStream_t>(stream), gain_dev,
                     (int)n, (int)m, match_out_dev, reinterpret_cast<long long*>(total_out_dev));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // extern "C"
