// Private to the library: the host functions that cross between the front door (gemm_f16.hip: which kernel serves a
// codetr_linear_* call, after its operand checks) and the translation units that own the three kernels.  Plain functions
// with hidden visibility (no part of the C ABI); bf16 is the operands' element type (false: fp16), and each owner
// dispatches to its templates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CODETR_GEMM_PRIVATE __attribute__((visibility("hidden")))

namespace gemm_route {

CODETR_GEMM_PRIVATE int launch_tile128(hipStream_t st, bool bf16, const void* X, const void* W, const void* bias,
                                       const void* R, void* Y, const void* mask, int M, int N, int K, int act, int hm_rows,
                                       int hm_hd);
CODETR_GEMM_PRIVATE bool big_applicable(int64_t M, int64_t N, int64_t K, int hm_hd);
CODETR_GEMM_PRIVATE int launch_tile256(hipStream_t st, bool bf16, const void* X, const void* W, const void* bias,
                                       const void* R, void* Y, const void* mask, int M, int N, int K, int act);
CODETR_GEMM_PRIVATE bool xs_applicable(int64_t M, int64_t N, int64_t K, int hm_hd);
CODETR_GEMM_PRIVATE int launch_xs(hipStream_t st, bool bf16, const void* X, const void* W, const void* bias, const void* R,
                                  void* Y, const void* mask, int M, int N, int K, int act, int hm_rows, int hm_hd);

}  // namespace gemm_route
