// Fused linear layer for MI355X (gfx950):  Y[M,N] = act(X[M,K] . W[N,K]^T + bias[N]) (+ R[M,N])
// fp16 / bf16 storage, fp32 accumulation on the matrix cores (v_mfma_f32_16x16x32_{f16,bf16}).
//
// This is the GEMM behind every nn.Linear of the Co-DETR hot path (Swin qkv / proj / MLP, encoder
// and decoder projections and FFNs, prediction heads: reference codetr/swin.py:91-115,
// codetr/transformer_mmcv.py:484-500, codetr/multi_scale_deformable_attention.py:173-213), with the
// bias add, ReLU/GELU and residual add that the reference runs as separate elementwise kernels
// folded into the epilogue.
//
// This file is the front door only: the operand checks of codetr_linear_{f16,bf16} and the rule that picks one of the
// three kernels behind them.  The kernels live in a translation unit each:
//   gemm_tile128.hip  128 x 128 LDS-staged tile (any M, N; also the implicit-GEMM convolution and split-K)
//   gemm_tile256.hip  256 x 256 tile for the large layers
//   gemm_xs.hip       X-stationary kernel for the short-K layers (and its LayerNorm / x + x2 / two-output forms)
// over gemm_tile.h (operand tiles in LDS, the launchers' host idiom) and gemm_epilogue.h (the output rule);
// gemm_route.h declares what crosses between them.  The persistent GEMMs (gemm_sk.hip, gemm_pp.hip) have entry
// points of their own.
//
// Requirements: K % 64 == 0, row pitches == K / N (dense row-major), 16-byte aligned bases.
// M and N are arbitrary (edge tiles clamp their loads and mask their stores).
#include "gemm_route.h"
#include "gemm_tile.h"

namespace {

// which of the three kernels behind codetr_linear_* serves a problem the front door has accepted (exported as
// codetr_linear_variant so hosts and tests can tell which kernel ran).  Only that: the entry points with a kernel form of
// their own (codetr_linear_ln_*, _xadd_*, _splitk_*, _sk_*, _pp_*, ...) check their domain themselves, and which entry
// point a layer calls is the host's routing (hip_ops.linear).  io16: Y (and R) 16-byte aligned.
enum { kKernel128 = 0, kKernel256 = 1, kKernelXS = 2 };
int pick_kernel(int64_t M, int64_t N, int64_t K, int act, bool has_res, int hm_hd, bool io16) {
  if (io16 && gemm_route::big_applicable(M, N, K, hm_hd)) return kKernel256;
  if (io16 && gemm_route::xs_applicable(M, N, K, hm_hd) && (K != 64 || (act == 0 && !has_res))) return kKernelXS;
  return kKernel128;
}

int launch(hipStream_t st, bool bf16, const void* X, const void* W, const void* bias, const void* R, void* Y,
           const void* mask, int64_t M, int64_t N, int64_t K, int act, int64_t hm_rows, int hm_hd) {
  if (!X || !W || !Y || M <= 0 || N <= 0 || K <= 0) return CODETR_E_BADARG;
  if (K % 64 != 0 || act < 0 || act > 3) return CODETR_E_UNSUPPORTED;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL || K > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (((M + BM - 1) / BM) * ((N + BN - 1) / BN) > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (act == 3 && !R) act = 1;   // ReLU after a residual that is not there
  if (!aligned16(X, W)) return CODETR_E_BADARG;
  if (hm_hd != 0 || hm_rows != 0) {
    if (hm_hd <= 0 || hm_rows <= 0 || hm_hd % 8 != 0 || N % hm_hd != 0 || N % 8 != 0 || M % hm_rows != 0 || R)
      return CODETR_E_UNSUPPORTED;
  }
  const bool io16 = aligned16(Y, R);
  const int kind = pick_kernel(M, N, K, act, R != nullptr, hm_hd, io16);
  if (kind == kKernel256) return gemm_route::launch_tile256(st, bf16, X, W, bias, R, Y, mask, (int)M, (int)N, (int)K, act);
  if (kind == kKernelXS)
    return gemm_route::launch_xs(st, bf16, X, W, bias, R, Y, mask, (int)M, (int)N, (int)K, act, (int)hm_rows, hm_hd);
  return gemm_route::launch_tile128(st, bf16, X, W, bias, R, Y, mask, (int)M, (int)N, (int)K, act, (int)hm_rows, hm_hd);
}

}  // namespace

extern "C" {

int codetr_linear_f16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                      const void* row_mask_dev, void* y_dev, int64_t M, int64_t N, int64_t K, int act, int64_t hm_rows,
                      int hm_head_dim) {
  return launch(static_cast<hipStream_t>(stream), false, x_dev, w_dev, bias_dev, residual_dev, y_dev, row_mask_dev, M,
                N, K, act, hm_rows, hm_head_dim);
}

int codetr_linear_bf16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev,
                       const void* residual_dev, const void* row_mask_dev, void* y_dev, int64_t M, int64_t N,
                       int64_t K, int act, int64_t hm_rows, int hm_head_dim) {
  return launch(static_cast<hipStream_t>(stream), true, x_dev, w_dev, bias_dev, residual_dev, y_dev, row_mask_dev, M, N,
                K, act, hm_rows, hm_head_dim);
}

const char* codetr_linear_variant(int64_t M, int64_t N, int64_t K, int act, int has_residual, int hm_head_dim) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64 != 0) return "unsupported";
  switch (pick_kernel(M, N, K, act, has_residual != 0, hm_head_dim, true)) {
    case kKernel256: return "tile256";
    case kKernelXS: return "xs";
    default: return "tile128";
  }
}

}  // extern "C"
