// The 128 x 128 tile kernel of the fused linear layer (gemm_f16.hip is the front door and says what the layer is):
// Y[M,N] = act(X[M,K] . W[N,K]^T + bias[N]) (+ R[M,N]), fp16 / bf16 storage, fp32 accumulation on the matrix cores.
// It serves every problem the other two kernels do not take, and in two further forms of the same tile loop the
// convolution on a token-major map as an implicit GEMM (codetr_conv_tokens_*) and the split-K pair
// (codetr_linear_splitk_*: fp32 partial tiles + a reduce kernel that applies the epilogue).
//
// Structure (cdna_hip_programming.md section 5, the 128x128 LDS-staged form):
//   * one 256-thread workgroup (4 waves, 2x2) owns a 128(M) x 128(N) output tile; each wave a
//     64x64 quadrant = 4x4 MFMA tiles of 16x16, K-step 64 (2 MFMAs deep per tile).
//   * both operands are K-contiguous (X rows, W rows), so both tiles are staged the same way:
//     global -> LDS with 16-byte LDS-DMA (lds_dma16, no VGPR round trip) into a ring
//     of 2-4 LDS buffers; up to 3 K-tiles stay in flight across the one raw s_barrier per K step
//     (counted wait_vmcnt), 64 KiB of LDS in every configuration -> 2 workgroups per CU.
//   * LDS image = [128 rows][8 x 16-B chunks]; the DMA destination is lane-linear, so the
//     bank-conflict swizzle is applied on the SOURCE address and undone on the fragment read:
//     chunk position = chunk ^ ((row >> 1) & 7)  -> the 16 rows of a ds_read_b128 lane group
//     land on 16 distinct 16-B slots of the 256-B bank row.
//   * operands are swapped (MFMA "A" = W tile, "B" = X tile) so that the accumulator layout puts
//     4 consecutive n of one output row m in each lane; the epilogue applies bias + activation on
//     the accumulators, passes the tile through LDS once and stores whole 128-byte lines
//     (16 B per lane) with the residual added on the way out.
//   * workgroup -> tile order is XCD-aware: each XCD walks a contiguous run of tiles, n fastest,
//     so the X rows shared by the tiles of one m-row come from one L2.
//
// Requirements: K % 64 == 0, row pitches == K / N (dense row-major), 16-byte aligned bases.
// M and N are arbitrary (edge tiles clamp their loads and mask their stores).
#include "gemm_route.h"
#include "gemm_tile.h"

namespace {

constexpr int kStagingBytes = 4 * 64 * kStagePitch;  // epilogue staging (gemm_epilogue.h): 36,864 B for the 4 waves

// ---- implicit im2col operand of codetr_conv_tokens_* ----------------------------------------------------------
// x [B, H, W, C] token-major, K ordered (ky, kx, c) with C % 64 == 0: a BKT-wide K slice (BKT <= 64) lies inside one
// tap (ky, kx), so each 16-byte piece of a staged X row is a piece of ONE shifted input pixel's C-vector, or zeros where
// the tap falls outside the map.  The zeros come from this buffer: LDS-DMA has no "write zeros" form, and one source
// that is always 128 readable zero bytes keeps the piece a single DMA instruction with the same vmcnt accounting as the
// dense tile.
__device__ __attribute__((aligned(16))) unsigned short g_conv_zeros[64];

struct ConvGeom {
  int H, W, C, Wo, HoWo, k, stride, pad;
};

// Per-thread state of the BKT/16 pieces a thread stages per X tile (the same piece -> (row, chunk) map as stage_tile):
// the piece's image base + chunk offset and the top-left input pixel of its output pixel.  Per K tile the tap is
// uniform, so a piece costs two adds, a bounds test and the DMA.
template <int BKT>
struct ConvRows {
  static constexpr int P = BKT / 16;
  const unsigned short* src[P];
  int iy[P], ix[P], chunk8[P];
  __device__ __forceinline__ void init(const unsigned short* X, const ConvGeom& g, int M, int m0, int tid) {
    constexpr int CH = BKT / 8;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int u = q * kThreads + tid;
      const int r = u / CH, pos = u % CH;
      chunk8[q] = (pos ^ sw<BKT>(r)) * 8;
      int m = m0 + r;
      m = m < M ? m : M - 1;  // edge tiles: re-read the last row, results masked later
      const int b = m / g.HoWo, p = m - b * g.HoWo;
      const int oy = p / g.Wo, ox = p - oy * g.Wo;
      src[q] = X + (size_t)b * g.H * g.W * g.C + chunk8[q];
      iy[q] = oy * g.stride - g.pad;
      ix[q] = ox * g.stride - g.pad;
    }
  }
  __device__ __forceinline__ void stage(const ConvGeom& g, int k0, unsigned char* lds_tile, int wave) const {
    const int tap = k0 / g.C, c0 = k0 - tap * g.C;
    const int ky = tap / g.k, kx = tap - ky * g.k;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int y = iy[q] + ky, x = ix[q] + kx;
      const unsigned short* s = ((unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W)
                                    ? src[q] + ((size_t)y * g.W + x) * g.C + c0
                                    : g_conv_zeros + chunk8[q];
      dma_piece(s, lds_tile, q, wave);
    }
  }
};

// ACT: 0 none, 1 relu, 2 gelu(erf), 3 relu after the residual.  BKT x STAGES = the K pipeline: STAGES LDS buffers of one (W tile, X tile)
// pair each, STAGES-1 tiles of LDS-DMA in flight across the per-K-step barrier (raw s_barrier + counted
// wait_vmcnt: a __syncthreads() would drain the DMA queue, cdna_hip_programming.md section 5).
// SPLITK: blockIdx.y picks a range of `kps` K tiles; the block's fp32 partial tile goes to Y viewed as
// float[gridDim.y][M][N] (no bias / activation / residual: splitk_reduce_kernel applies them to the sum).
// CONV: X is not a dense [M, K] matrix but the implicit im2col matrix of a convolution over a token-major map (ConvRows
// below); the tile loop, the W side and the epilogue are the same code.
template <class T, int ACT, bool HAS_BIAS, bool HAS_RES, int BKT, int STAGES, bool SPLITK, bool CONV>
__device__ __forceinline__ void linear_body(const unsigned short* __restrict__ X, const unsigned short* __restrict__ W,
                                            const unsigned short* __restrict__ bias,
                                            const unsigned short* __restrict__ R, unsigned short* __restrict__ Y,
                                            const unsigned char* __restrict__ row_mask, int M, int N, int K,
                                            int tiles_n, int hm_rows, int hm_hd, int kps, const ConvGeom& cg) {
  constexpr int kTileBytes = 128 * BKT * 2;        // one operand tile
  constexpr int kStageBytes = 2 * kTileBytes;      // W tile + X tile
  constexpr int LPS = 2 * (BKT / 16);              // LDS-DMA instructions per thread per stage
  constexpr int kLdsBytes = STAGES * kStageBytes > kStagingBytes ? STAGES * kStageBytes : kStagingBytes;
  static_assert(kLdsBytes <= 64 * 1024, "pipeline does not fit 64 KiB");
  static_assert(STAGES >= 2 && STAGES <= 4, "");
  // one object only (a second __shared__ object de-pipelines LDS-DMA kernels); the epilogue staging reuses it
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;  // wave quadrant inside the 128x128 tile

  const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
  const int tn = tile % tiles_n, tm = tile / tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // The accumulators start at the bias (D = A.B + C with C = bias broadcast along m): the bias add costs nothing
  // and its load latency hides under the first K stage.  A lane's 4 registers of tile (i, j) are the 4 consecutive
  // output columns n = wn*64 + i*16 + 4*(lane>>4) + r, the same for every j.
  const int ncol = 4 * (lane >> 4);
  const bool vec_n = (N & 7) == 0;
  f32x4 acc[4][4];  // [n-tile][m-tile]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (HAS_BIAS) {
      const int n = n0 + wn * 64 + i * 16 + ncol;
      if (vec_n) {
        if (n < N) {
          const s16x4 bb = *reinterpret_cast<const s16x4*>(bias + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) b4[r] = T::to_f32((unsigned short)bb[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) b4[r] = T::to_f32(bias[n + r]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = b4;
  }

  const int kt0 = SPLITK ? (int)blockIdx.y * kps : 0;
  const int nk = SPLITK ? (K / BKT - kt0 < kps ? K / BKT - kt0 : kps) : K / BKT;
  const int frow = lane & 15, fchunk = lane >> 4;
  constexpr int KS = BKT / 32;
  ConvRows<BKT> crows;
  if (CONV) crows.init(X, cg, M, m0, tid);
  {
  auto issue = [&](int t) {
    unsigned char* buf = lds + (t % STAGES) * kStageBytes;
    stage_tile<BKT>(W, N, K, n0, (kt0 + t) * BKT, buf, tid);
    if (CONV) crows.stage(cg, (kt0 + t) * BKT, buf + kTileBytes, wave);
    else stage_tile<BKT>(X, M, K, m0, (kt0 + t) * BKT, buf + kTileBytes, tid);
  };
#pragma unroll
  for (int s0 = 0; s0 < STAGES - 1; ++s0)
    if (s0 < nk) issue(s0);

  for (int t = 0; t < nk; ++t) {
    // tiles issued beyond t: t+1 .. min(nk-1, t+STAGES-2); tile t itself must have landed
    const int ahead = (nk - 1 < t + STAGES - 2 ? nk - 1 : t + STAGES - 2) - t;
    if (STAGES >= 4 && ahead == 2) wait_vmcnt<2 * LPS>();
    else if (STAGES >= 3 && ahead == 1) wait_vmcnt<LPS>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // everyone's part of tile t is in LDS; everyone is done reading tile t-1
    if (t + STAGES - 1 < nk) issue(t + STAGES - 1);  // overwrites the buffer of tile t-1
    const unsigned char* bufW = lds + (t % STAGES) * kStageBytes;
    const unsigned char* bufX = bufW + kTileBytes;
    typename T::frag a[2][4], b[2][4];
    auto read_frags = [&](int ks, int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) a[buf][i] = read_frag<T, BKT>(bufW, wn * 64 + i * 16 + frow, ks * 4 + fchunk);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[buf][j] = read_frag<T, BKT>(bufX, wm * 64 + j * 16 + frow, ks * 4 + fchunk);
    };
    read_frags(0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 1 < KS) read_frags(ks + 1, (ks + 1) & 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = T::mfma(a[ks & 1][i], b[ks & 1][j], acc[i][j]);
      if (ks + 1 < KS) {
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
      } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      }
    }
  }
  }
  __builtin_amdgcn_s_barrier();  // all fragment reads done (no DMA is in flight any more): LDS is free for the epilogue

  if (SPLITK) {
    float* part = reinterpret_cast<float*>(Y) + (size_t)blockIdx.y * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + wn * 64 + i * 16 + ncol;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + j * 16 + frow;
        if (m >= M || n >= N) continue;
        if (vec_n) {
          *reinterpret_cast<f32x4*>(part + (size_t)m * N + n) = acc[i][j];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < N) part[(size_t)m * N + n + r] = acc[i][j][r];
        }
      }
    }
    return;
  }

  // ---- epilogue: the output rule of gemm_epilogue.h ------------------------------------------------
  // accumulator layout: for MFMA tile (i, j) a lane holds n = wn*64 + i*16 + 4*(lane>>4) + r (r = 0..3),
  // m = wm*64 + j*16 + (lane&15), i.e. 8 contiguous output bytes per lane and 32-byte row segments per
  // store instruction.  Partial-line stores of that shape run at ~1 TB/s, so the tile goes through LDS
  // once and leaves as whole 128-byte lines (16 B per lane): activation in fp32 on the accumulators ->
  // 16-bit image of the wave's 64x64 quadrant in its private LDS region -> read back by rows, row state,
  // residual -> global_store_dwordx4.
  if (vec_n) {
    constexpr int kPitch = kStagePitch;  // bytes per staged row (+16: rows 0/8 do not share a bank pair)
    unsigned char* stage = lds + wave * (64 * kPitch);  // main loop is done with LDS (barrier above)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = epi_act<ACT, HAS_RES>(acc[i][j][r]);
        *reinterpret_cast<s16x4*>(stage + (j * 16 + frow) * kPitch + (i * 16 + ncol) * 2) = T::pack4(v);
      }
    }
    __builtin_amdgcn_wave_barrier();  // same wave writes then reads: DS ops retire in order
    const int srow = lane >> 3, schunk = lane & 7;
    const int n = n0 + wn * 64 + schunk * 8;
    // residual rows, all requested before the first use (one exposed latency instead of eight); the head-major
    // destination never carries a residual
    s16x8 rres[8];
    if (HAS_RES) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        int m = m0 + wm * 64 + it * 8 + srow;
        m = m < M ? m : M - 1;
        // epi_residual_col with the guard this kernel has always compiled (N % 8 == 0 here, so N >= 8 and the guard is dead)
        const int nn = n + 8 <= N ? n : (N >= 8 ? N - 8 : 0);
        rres[it] = *reinterpret_cast<const s16x8*>(R + (size_t)m * N + nn);
      }
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int ml = it * 8 + srow;
      const int m = m0 + wm * 64 + ml;
      if (m < M && n < N) {
        s16x8 v = *reinterpret_cast<const s16x8*>(stage + ml * kPitch + schunk * 16);
        if (row_mask) {
          // epi_row_state written out: through the helper this kernel's forms with a bias compiled to other instructions
          const unsigned char mk = row_mask[m];
          if (mk == 2) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              v[e] = (short)T::from_f32(epi_act<ACT, HAS_RES>(HAS_BIAS ? T::to_f32(bias[n + e]) : 0.f));
          } else if (mk) {
            v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
          }
        }
        size_t off = (size_t)m * N + n;
        if (hm_hd > 0) off = epi_head_major(m, n, N, hm_rows, hm_hd);
        if (HAS_RES) {
          const s16x8 rr = rres[it];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = (short)epi_residual<T, ACT>((unsigned short)v[e], (unsigned short)rr[e]);
        }
        *reinterpret_cast<s16x8*>(Y + off) = v;
      }
    }
    return;
  }
  // ragged N (N % 8 != 0: the 4-wide box head, test shapes): direct stores from the accumulator layout
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + i * 16 + ncol;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + wm * 64 + j * 16 + frow;
      if (m >= M) continue;
      const size_t off = (size_t)m * N + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (n + r < N) {
          unsigned short h = T::from_f32(epi_act<ACT, HAS_RES>(acc[i][j][r]));
          if (row_mask) epi_row_state<T, T, ACT, HAS_RES>(h, row_mask[m], HAS_BIAS, bias, n + r);
          if (HAS_RES) h = epi_residual<T, ACT>(h, R[off + r]);
          Y[off + r] = h;
        }
      }
    }
  }
}

template <class T, int ACT, bool HAS_BIAS, bool HAS_RES, int BKT, int STAGES, bool SPLITK = false>
__global__ __launch_bounds__(kThreads) void linear_kernel(const unsigned short* __restrict__ X,
                                                          const unsigned short* __restrict__ W,
                                                          const unsigned short* __restrict__ bias,
                                                          const unsigned short* __restrict__ R,
                                                          unsigned short* __restrict__ Y,
                                                          const unsigned char* __restrict__ row_mask, int M, int N,
                                                          int K, int tiles_n, int hm_rows, int hm_hd, int kps) {
  linear_body<T, ACT, HAS_BIAS, HAS_RES, BKT, STAGES, SPLITK, false>(X, W, bias, R, Y, row_mask, M, N, K, tiles_n,
                                                                     hm_rows, hm_hd, kps, ConvGeom{});
}

// Convolution on a token-major map as an implicit GEMM (codetr_conv_tokens_*): rows m = output pixels (b, oy, ox),
// K = (ky, kx, c), W = conv.weight permuted to [Cout, k k C]; y [B, Ho, Wo, Cout] is the GEMM's [M, N] result.
template <class T, int ACT, bool HAS_BIAS, bool HAS_RES, int BKT, int STAGES>
__global__ __launch_bounds__(kThreads) void conv_tokens_kernel(const unsigned short* __restrict__ X,
                                                               const unsigned short* __restrict__ W,
                                                               const unsigned short* __restrict__ bias,
                                                               const unsigned short* __restrict__ R,
                                                               unsigned short* __restrict__ Y, int M, int N, int K,
                                                               int tiles_n, ConvGeom cg) {
  linear_body<T, ACT, HAS_BIAS, HAS_RES, BKT, STAGES, false, true>(X, W, bias, R, Y, nullptr, M, N, K, tiles_n, 0, 0, 0,
                                                                   cg);
}

// Pipeline configuration per problem (A/B on MI355X over the model's 22 layer shapes, tools/bench_linear.py):
//   K <= 256 (every 256-wide transformer layer, Swin stage 0): 32-deep K steps, 2 buffers -> 36 KiB of LDS, 3
//     workgroups per CU.  These layers run 4-8 K steps per tile; their cost is the per-tile fixed latency
//     (first loads, bias, LDS staging, stores), which only more resident workgroups hide.
//   K  > 256: 64-deep steps, 2 buffers (64 KiB, 2 workgroups per CU): twice the MFMA work per barrier.
//   A 4-deep ring (3 tiles of DMA in flight, counted vmcnt) measured 5-10 % slower than either on every shape, and
//   a persistent-grid variant that prefetched the next tile's first stage under the epilogue 20 % slower: ablation
//   (stores off / K loop off) shows the short-K layers bound by bytes through the CU's vector-memory path --
//   L2->LDS operand re-reads (3.35 GB at ~17 TB/s for the encoder FFN up-projection) + staging + stores -- not by
//   exposed latency.  The lever that remains is a larger tile (fewer operand re-reads); see DESIGN.md section 4.
//   Grids of at most one workgroup per CU (the decoder's 900-query layers: 16 tiles) gain nothing from occupancy;
//     their time is the chain of per-K-step DMA latencies, so they take the 64-deep step (half the steps) as well.
// (The A/B overrides of this choice -- a 4-deep ring, the DMA pieces spread over the MFMAs -- measured slower on every
// shape in rounds 1-3 and are gone from the library; profiles/r02_*, r03_gemm256_ablation.txt keep the numbers.)
int pipeline_cfg(int64_t K, int64_t tiles) { return (K <= 256 && tiles > 256) ? 322 : 642; }

template <class T, int ACT, int BKT, int STAGES>
int launch_cfg(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y,
               const void* mask, int M, int N, int K, int hm_rows, int hm_hd) {
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(kThreads);
  const Operands o(X, W, bias, R, Y, mask);
  dispatch_bias_res(bias, R, [&](auto hb, auto hr) {
    hipLaunchKernelGGL((linear_kernel<T, ACT, hb(), hr(), BKT, STAGES, false>), grid, block, 0, st, o.x, o.w, o.b, o.r, o.y,
                       o.mk, M, N, K, tiles_n, hm_rows, hm_hd, 0);
  });
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

// y = act(sum_z part[z] + bias) (masked rows -> 0) + residual, 4 columns per thread
template <class T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part,
                                                            const unsigned short* __restrict__ bias,
                                                            const unsigned short* __restrict__ R,
                                                            const unsigned char* __restrict__ row_mask,
                                                            unsigned short* __restrict__ Y, int M, int N, int splits,
                                                            int act) {
  const int ngroups = (N + 3) / 4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M * ngroups) return;
  const int m = (int)(idx / ngroups), n = (int)(idx % ngroups) * 4;
  const size_t off = (size_t)m * N + n;
  const bool vec = (N & 3) == 0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < splits; ++z) {
    const float* p = part + (size_t)z * M * N + off;
    if (vec) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += q[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) v[r] += p[r];
    }
  }
  const unsigned char mk = row_mask ? row_mask[m] : 0;
  dispatch_act(act, [&](auto a) {   // (act <= 2: the residual plays no part in the activation)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (n + r >= N) break;
      unsigned short h = T::from_f32(epi_act<a(), false>(v[r] + (bias ? T::to_f32(bias[n + r]) : 0.f)));
      epi_row_state<T, T, a(), false>(h, mk, bias != nullptr, bias, n + r);
      if (R) h = epi_residual<T, 0>(h, R[off + r]);
      Y[off + r] = h;
    }
  });
}

// Split-K plan: problems whose 128x128 output tiles cannot fill the chip but whose K is long (the neck's extra
// 3x3/s2 level as a GEMM: 600 x 256 x 13824 = 10 tiles, 183 us in one pass) are cut along K into `splits` ranges of
// whole 64-wide K tiles so that ~1.5 blocks per CU are in flight.  Returns 1 when a single pass is the better launch.
int splitk_plan(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN), ktiles = K / 64;
  if (tiles > 128 || K < 2048 || K % 64 != 0) return 1;
  // 65 ... 128 tiles (Swin stage-2 fc2 of a 608x608 image: 72 tiles x 48 k-tiles; stage-3 fc2 of a 1152x768 image: 84 x 96):
  // as many whole passes over K as still fit one round of the chip
  int64_t splits = tiles > 64 ? 256 / tiles : (384 + tiles - 1) / tiles;
  if (splits > ktiles / 4) splits = ktiles / 4;
  if (splits < 2) return 1;
  const int64_t kps = (ktiles + splits - 1) / splits;
  return (int)((ktiles + kps - 1) / kps);
}

template <class T>
int launch_splitk(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y,
                  const void* mask, int64_t M, int64_t N, int64_t K, int act, int splits, void* ws, int64_t ws_bytes) {
  if (!X || !W || !Y || !ws || M <= 0 || N <= 0 || K <= 0 || splits < 2) return CODETR_E_BADARG;
  if (K % 64 != 0 || act < 0 || act > 2) return CODETR_E_UNSUPPORTED;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL || K > 0x7fffffffLL || splits > 65535) return CODETR_E_TOO_LARGE;
  if (!aligned16(X, W, ws)) return CODETR_E_BADARG;
  if (ws_bytes < (int64_t)splits * M * N * 4) return CODETR_E_BADARG;
  const int ktiles = (int)(K / 64), kps = (ktiles + splits - 1) / splits;
  if ((int64_t)kps * (splits - 1) >= ktiles) return CODETR_E_BADARG;  // an empty last range
  const int tiles_m = (int)((M + BM - 1) / BM), tiles_n = (int)((N + BN - 1) / BN);
  const dim3 grid((unsigned)(tiles_m * tiles_n), (unsigned)splits), block(kThreads);
  const Operands o(X, W, bias, R, Y, mask);
  hipLaunchKernelGGL((linear_kernel<T, 0, false, false, 64, 2, true>), grid, block, 0, st, o.x, o.w, nullptr, nullptr,
                     static_cast<unsigned short*>(ws), nullptr, (int)M, (int)N, (int)K, tiles_n, 0, 0, kps);
  const long groups = (long)M * ((N + 3) / 4);
  hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
                     static_cast<const float*>(ws), o.b, o.r, o.mk, o.y, (int)M, (int)N, splits, act);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

template <class T, int ACT, int BKT>
int launch_conv_cfg(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y, int M, int N,
                    int K, const ConvGeom& g) {
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(kThreads);
  const Operands o(X, W, bias, R, Y);
  dispatch_bias_res(bias, R, [&](auto hb, auto hr) {
    hipLaunchKernelGGL((conv_tokens_kernel<T, ACT, hb(), hr(), BKT, 2>), grid, block, 0, st, o.x, o.w, o.b, o.r, o.y, M, N, K,
                       tiles_n, g);
  });
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

template <class T>
int launch_conv(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y, int64_t B,
                int64_t H, int64_t Wd, int64_t C, int64_t Cout, int k, int stride, int pad, int act) {
  if (!X || !W || !Y || B <= 0 || H <= 0 || Wd <= 0 || C <= 0 || Cout <= 0) return CODETR_E_BADARG;
  if ((k != 1 && k != 3) || (stride != 1 && stride != 2) || pad < 0 || pad >= k || C % 64 != 0 || Cout % 8 != 0 ||
      act < 0 || act > 3)
    return CODETR_E_UNSUPPORTED;
  if (!aligned16(X, W, Y, R, bias)) return CODETR_E_BADARG;
  const int64_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (Wd + 2 * pad - k) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return CODETR_E_BADARG;
  const int64_t M = B * Ho * Wo, K = (int64_t)k * k * C;
  if (M > 0x7fffffffLL || Cout > 0x7fffffffLL || K > 0x7fffffffLL || H > 0xffffLL || Wd > 0xffffLL)
    return CODETR_E_TOO_LARGE;
  if (((M + BM - 1) / BM) * ((Cout + BN - 1) / BN) > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (act == 3 && !R) act = 1;
  const ConvGeom g{(int)H, (int)Wd, (int)C, (int)Wo, (int)(Ho * Wo), k, stride, pad};
  // the linear's pipeline rule (a K slice of 32 or 64 stays inside one tap: C % 64 == 0)
  const bool short_k = pipeline_cfg(K, ((M + BM - 1) / BM) * ((Cout + BN - 1) / BN)) == 322;
  return dispatch_act(act, [&](auto a) {
    if (short_k) return launch_conv_cfg<T, a(), 32>(st, X, W, bias, R, Y, (int)M, (int)Cout, (int)K, g);
    return launch_conv_cfg<T, a(), 64>(st, X, W, bias, R, Y, (int)M, (int)Cout, (int)K, g);
  });
}

}  // namespace

int gemm_route::launch_tile128(hipStream_t st, bool bf16, const void* X, const void* W, const void* bias, const void* R,
                               void* Y, const void* mask, int M, int N, int K, int act, int hm_rows, int hm_hd) {
  const bool short_k = pipeline_cfg(K, (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN)) == 322;
  return dispatch_elem(bf16, [&](auto t) {
    return dispatch_act(act, [&](auto a) {
      if (short_k) return launch_cfg<decltype(t), a(), 32, 2>(st, X, W, bias, R, Y, mask, M, N, K, hm_rows, hm_hd);
      return launch_cfg<decltype(t), a(), 64, 2>(st, X, W, bias, R, Y, mask, M, N, K, hm_rows, hm_hd);
    });
  });
}

extern "C" {

int codetr_conv_tokens_f16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev,
                           const void* residual_dev, void* y_dev, int64_t B, int64_t H, int64_t W, int64_t C,
                           int64_t Cout, int k, int stride, int pad, int act) {
  return launch_conv<HalfT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev, B, H, W, C,
                            Cout, k, stride, pad, act);
}

int codetr_conv_tokens_bf16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev,
                            const void* residual_dev, void* y_dev, int64_t B, int64_t H, int64_t W, int64_t C,
                            int64_t Cout, int k, int stride, int pad, int act) {
  return launch_conv<BFloatT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev, B, H, W, C,
                              Cout, k, stride, pad, act);
}

int codetr_linear_splitk_plan(int64_t M, int64_t N, int64_t K, int64_t* workspace_bytes) {
  const int splits = splitk_plan(M, N, K);
  if (workspace_bytes) *workspace_bytes = splits > 1 ? (int64_t)splits * M * N * 4 : 0;
  return splits;
}

int codetr_linear_splitk_f16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev,
                             const void* residual_dev, const void* row_mask_dev, void* y_dev, int64_t M, int64_t N,
                             int64_t K, int act, int splits, void* workspace_dev, int64_t workspace_bytes) {
  return launch_splitk<HalfT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev,
                              row_mask_dev, M, N, K, act, splits, workspace_dev, workspace_bytes);
}

int codetr_linear_splitk_bf16(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev,
                              const void* residual_dev, const void* row_mask_dev, void* y_dev, int64_t M, int64_t N,
                              int64_t K, int act, int splits, void* workspace_dev, int64_t workspace_bytes) {
  return launch_splitk<BFloatT>(static_cast<hipStream_t>(stream), x_dev, w_dev, bias_dev, residual_dev, y_dev,
                                row_mask_dev, M, N, K, act, splits, workspace_dev, workspace_bytes);
}

}  // extern "C"
