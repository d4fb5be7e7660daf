// The 256 x 256 tile kernel of the fused linear layer (gemm_f16.hip is the front door and says what the layer is):
// Y[M,N] = act(X[M,K] . W[N,K]^T + bias[N]) (+ R[M,N]), fp16 / bf16 storage, fp32 accumulation on the matrix cores,
// for K >= 256, N % 8 == 0 and grids of at least 200 tiles (big_applicable below).
//
// 256 x 256 tile for the large layers (Swin stages 2-3 at 8 images per GPU: M = 77-81 k rows).  A 128 x 128 x 64 tile
// step moves 32 KB of operands through the CU's vector-memory path per 2.1 MFLOP -- 64 B/clk per CU at MFMA peak,
// which IS that path's rate, so the 128-tile kernel (gemm_tile128.hip) tops out near 0.9 PF while hipBLASLt's 256-wide
// macro tiles reach 1.1-1.4 PF on these shapes.  Here: 512 threads = 8 waves (2 along m x 4 along n), each wave
// 128(m) x 64(n) = 8 x 4 MFMA tiles (128 accumulator registers); one workgroup per CU (all 160 KiB of its LDS: operand
// tiles of 256 x 64, see the ring below); 32 B/clk per CU of operand traffic and 12 fragment reads per 32 MFMAs.  Same
// LDS image, swizzle, bias-in-accumulator and LDS-staged epilogue (in two 64-row halves) as linear_kernel.
// Ablation at 8 images (M = 80 640, us): main loop only / full kernel = qkv 287 / 379, proj+res 87 / 161, fc1+GELU
// 314 / 520, fc2+res 355 / 412 -- the main loop runs at 1.0-1.15 PF (hipBLASLt: 1.1-1.2 PF including its store), the
// epilogue costs 25-40 % on top.  Two attempts to hide it, both measured slower and removed: (a) a 256 x 128 / 4-wave /
// BK 32 variant with two workgroups per CU so that one's epilogue overlaps the other's MFMAs (423 vs 384 us on qkv:
// the main loop loses more than the overlap returns); (b) a persistent variant that parks the finished fp16 tile in
// 96 KiB of LDS + 16 registers and writes it back one store per K step of the next tile, with the stores allowed to
// stay in flight across barriers (450 vs 376 us: the write-back costs the same trickled as in bulk, so it is not
// issue latency -- most likely the 372 MB of output passing through the L2 / Infinity Cache evicts the activation
// rows every column tile re-reads).  Next thing to try: non-temporal stores with a column-major tile walk.
#include "gemm_route.h"
#include "gemm_tile.h"

namespace {

#ifdef CODETR_GEMM_STAMPS
__device__ unsigned long long* g_stamps = nullptr;
#endif
// diagnostic builds only (tools/micro/gemm256_stamps.hip -DCODETR_GEMM_ABL=mask; WRONG results by construction):
// 1 = no LDS-DMA inside the main loop, 2 = no MFMAs, 4 = no fragment reads, 8 = no wait + barrier per k-tile
#ifdef CODETR_GEMM_ABL
constexpr int kGemmAbl = CODETR_GEMM_ABL;
#else
constexpr int kGemmAbl = 0;
#endif
// The operand ring, [X0 X1 X2][W0 W1] = 5 tiles of 32 KiB = 160 KiB, the whole LDS of the CU: the X operand (the one that
// misses L2 more: each 256-row slice is shared by the N/256 column tiles only, the W slices by every row tile) is
// prefetched TWO k-tiles ahead through a 3-slot ring; W stays one tile ahead in its 2-slot ring.  The form this replaced
// (removed; a template parameter XDEEP chose between the two) was a 2-stage ring [W0 X0][W1 X1] of 128 KiB with both
// operands one tile ahead: in-kernel stamps (tools/micro/gemm256_stamps.hip) showed that loop waiting for its LDS-DMA
// ~48 % of the time at 8 images (4300 cycles per k-tile against 2050 of MFMA work): the operand fetch takes ~2 us under
// load and only one tile time was there to hide it (profiles/r02_gemm256_stamps.txt, r02_gemm256_xdeep_ab.txt keep the
// numbers: -3 ... -13 % on every Swin stage 1-3 shape at 8 images).
template <class T, int ACT, bool HAS_BIAS, bool HAS_RES, bool SDMA>
__global__ __launch_bounds__(512) void linear_256_kernel(const unsigned short* __restrict__ X,
                                                         const unsigned short* __restrict__ W,
                                                         const unsigned short* __restrict__ bias,
                                                         const unsigned short* __restrict__ R,
                                                         unsigned short* __restrict__ Y,
                                                         const unsigned char* __restrict__ row_mask, int M, int N, int K,
                                                         int tiles_n) {
  constexpr int BKT = 64, NT = 512;
#ifdef CODETR_GEMM_STAMPS   // diagnostic build only (tools/micro/gemm256_stamps.hip): in-kernel timeline of every workgroup
  unsigned long long st0 = 0, st1 = 0, st2 = 0, rt0 = 0;
  if (threadIdx.x == 0) {
    st0 = __builtin_amdgcn_s_memtime();
    rt0 = __builtin_amdgcn_s_memrealtime();
  }
#endif
  constexpr int kTileBytes = 256 * BKT * 2;   // 32 KiB: one operand tile
  // [X0 X1 X2][W0 W1] (160 KiB, the whole LDS of the CU)
  __shared__ __attribute__((aligned(16))) unsigned char lds[5 * kTileBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
  const int tn = tile % tiles_n, tm = tile / tiles_n;
  const int m0 = tm * 256, n0 = tn * 256;
  const int frow = lane & 15, fchunk = lane >> 4, ncol = 4 * (lane >> 4);

  f32x4 acc[4][8];  // [n-tile][m-tile]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (HAS_BIAS) {
      const int n = n0 + wn * 64 + i * 16 + ncol;
      if (n < N) {  // N % 8 == 0 on this path
        const s16x4 bb = *reinterpret_cast<const s16x4*>(bias + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) b4[r] = T::to_f32((unsigned short)bb[r]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = b4;
  }

  // per-thread source pointers of the 4 + 4 LDS-DMA pieces of a stage (piece q covers rows q*64 + tid/8)
  const unsigned short* gw[4];
  const unsigned short* gx[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = q * 64 + (tid >> 3), pos = tid & 7;
    const int chunk = pos ^ sw<BKT>(r);
    int gn = n0 + r, gm = m0 + r;
    gn = gn < N ? gn : N - 1;
    gm = gm < M ? gm : M - 1;
    gw[q] = W + (size_t)gn * K + chunk * 8;
    gx[q] = X + (size_t)gm * K + chunk * 8;
  }
  // SDMA: the same pieces addressed as (wave-uniform 64-bit base of the tile's first row and k-tile, in SGPRs) + (per-thread
  // 32-bit byte offset, fixed for the whole tile): the LDS-DMA is then one inline-assembly instruction per piece -- no
  // 64-bit vector add, no v_readfirstlane for its LDS destination, eight address registers less (the pointer form spilled
  // two registers that were reloaded inside the loop, and a scratch reload counts in vmcnt: the counted wait then asked
  // for half of the tile that was meant to stay in flight)
  unsigned woff[4], xoff[4];
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const unsigned char* Wt = reinterpret_cast<const unsigned char*>(W) + (size_t)n0 * K * 2;
  const unsigned char* Xt = reinterpret_cast<const unsigned char*>(X) + (size_t)m0 * K * 2;
  if (SDMA) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = q * 64 + (tid >> 3), pos = tid & 7;
      const int chunk = pos ^ sw<BKT>(r);
      const int rn = n0 + r < N ? r : N - 1 - n0, rm = m0 + r < M ? r : M - 1 - m0;   // edge tiles: the last row again
      woff[q] = (unsigned)((rn * K + chunk * 8) * 2);
      xoff[q] = (unsigned)((rm * K + chunk * 8) * 2);
    }
  }
  auto sdmaW = [&](int q, int kt, unsigned char* slot) {
    lds_dma16(Wt + (size_t)kt * (BKT * 2), woff[q], slot + (q * NT + wave_u * 64) * 16);
  };
  auto sdmaX = [&](int q, int kt, unsigned char* slot) {
    lds_dma16(Xt + (size_t)kt * (BKT * 2), xoff[q], slot + (q * NT + wave_u * 64) * 16);
  };
  const int nk = K / BKT;
  // k-tile index of loop step i (steps past the end re-fetch the last one).  A per-tile rotation of this walk (so that
  // tiles sharing an operand slice do not ask for it at the same moment) was measured neutral to -6 % and removed
  // (profiles/r03_gemm256_ablation.txt).
  auto ktile = [&](int i) { return i < nk ? i : nk - 1; };
  if (SDMA) {
#pragma unroll
    for (int q = 0; q < 4; ++q) sdmaW(q, ktile(0), lds + 3 * kTileBytes);
#pragma unroll
    for (int q = 0; q < 4; ++q) sdmaX(q, ktile(0), lds);
#pragma unroll
    for (int q = 0; q < 4; ++q) sdmaX(q, ktile(1), lds + kTileBytes);
  } else {   // issue order W(0), X(0), X(1): the youngest four pieces may stay in flight at the first wait
    const size_t k0 = (size_t)ktile(0) * BKT;
#pragma unroll
    for (int q = 0; q < 4; ++q) lds_dma16_auto(gw[q] + k0, lds + 3 * kTileBytes + (q * NT + wave * 64) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) lds_dma16_auto(gx[q] + k0, lds + (q * NT + wave * 64) * 16);
    const size_t k1 = (size_t)ktile(1) * BKT;
#pragma unroll
    for (int q = 0; q < 4; ++q) lds_dma16_auto(gx[q] + k1, lds + kTileBytes + (q * NT + wave * 64) * 16);
  }
#ifdef CODETR_GEMM_STAMPS
  unsigned long long wait_dma = 0, wait_bar = 0;
#endif
  int xs = 0;  // ring slot of X(t)
  for (int t = 0; t < nk; ++t) {
#ifdef CODETR_GEMM_STAMPS
    const unsigned long long w0 = __builtin_amdgcn_s_memtime();
    wait_vmcnt<4>();
    const unsigned long long w1 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_barrier();
    const unsigned long long w2 = __builtin_amdgcn_s_memtime();
    wait_dma += w1 - w0;
    wait_bar += w2 - w1;
#else
    if (!(kGemmAbl & 8)) {
      wait_vmcnt<4>();   // W(t) and X(t) have landed; the four pieces of X(t+1) may still be in flight
      __builtin_amdgcn_s_barrier();  // tile t is in LDS for everyone; everyone is done reading tile t-1
    }
#endif
    const unsigned char* bufW = lds + (3 + (t & 1)) * kTileBytes;
    const unsigned char* bufX = lds + xs * kTileBytes;
    // One workgroup per CU: its 8 waves reach this point together, so nothing else covers a burst of DMA issue or an
    // LDS wait.  The schedule is pinned: fragments of k-step 1 are read behind the first two MFMAs of step 0, and the
    // 8 DMA pieces of tile t+1 go out one per 3 MFMAs of step 0 (early enough to land under step 1).  Past the last
    // tile the pieces re-fetch it into the idle buffer (no branch in the pinned region); drained before the epilogue.
    const size_t koff = (size_t)ktile(t + 1) * BKT;
    // W(t+1) -> the W slot tile t-1 used, X(t+2) -> the X slot tile t-1 used (re-fetches of the last tile past
    // the end keep the in-flight count uniform)
    const size_t koffx = (size_t)ktile(t + 2) * BKT;
    unsigned char* nbufW = lds + (3 + ((t + 1) & 1)) * kTileBytes;
    const int xs2 = xs >= 1 ? xs - 1 : 2;   // (xs + 2) % 3
    unsigned char* nbufX = lds + xs2 * kTileBytes;
    xs = xs == 2 ? 0 : xs + 1;
#ifdef CODETR_GEMM_ABL
    typename T::frag a[2][4] = {}, b[2][8] = {};
#else
    typename T::frag a[2][4], b[2][8];
#endif
    auto read_frags = [&](int ks, int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) a[buf][i] = read_frag<T, BKT>(bufW, wn * 64 + i * 16 + frow, ks * 4 + fchunk);
#pragma unroll
      for (int j = 0; j < 8; ++j) b[buf][j] = read_frag<T, BKT>(bufX, wm * 128 + j * 16 + frow, ks * 4 + fchunk);
    };
    if (SDMA) {
      // explicit interleave (the inline-assembly pieces are opaque to sched_group_barrier): step-0 fragments, the first two
      // MFMAs, the step-1 fragments, then eight groups of (3 MFMAs, 1 piece) -- W(t+1) first, it is needed one tile from
      // now, X(t+2) two -- each closed by a scheduling barrier; then the remaining 6 + 32 MFMAs
      read_frags(0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
      read_frags(1, 1);
      auto mf0 = [&](int idx) {
        const int j = idx >> 2, i = idx & 3;
        acc[i][j] = T::mfma(a[0][i], b[0][j], acc[i][j]);
      };
      mf0(0);
      mf0(1);
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
      __builtin_amdgcn_sched_barrier(0);
      const int ktw = ktile(t + 1), ktx = ktile(t + 2);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        mf0(2 + 3 * g);
        mf0(3 + 3 * g);
        mf0(4 + 3 * g);
        if (g < 4) sdmaW(g, ktw, nbufW);
        else sdmaX(g - 4, ktx, nbufX);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int idx = 26; idx < 32; ++idx) mf0(idx);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = T::mfma(a[1][i], b[1][j], acc[i][j]);
      __builtin_amdgcn_sched_group_barrier(0x008, 38, 0);
      continue;
    }
    if (!(kGemmAbl & 4)) read_frags(0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
    // ---- k-step 0 ----
    if (!(kGemmAbl & 4)) read_frags(1, 1);
    if (!(kGemmAbl & 1)) {   // W first: it is needed one tile from now, X two
#pragma unroll
      for (int q = 0; q < 4; ++q) lds_dma16_auto(gw[q] + koff, nbufW + (q * NT + wave * 64) * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) lds_dma16_auto(gx[q] + koffx, nbufX + (q * NT + wave * 64) * 16);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!(kGemmAbl & 2)) acc[i][j] = T::mfma(a[0][i], b[0][j], acc[i][j]);
        else if (!(kGemmAbl & 4)) asm volatile("" ::"v"(a[0][i]), "v"(b[0][j]));
      }
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
    // ---- k-step 1 ----
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!(kGemmAbl & 2)) acc[i][j] = T::mfma(a[1][i], b[1][j], acc[i][j]);
        else if (!(kGemmAbl & 4)) asm volatile("" ::"v"(a[1][i]), "v"(b[1][j]));
      }
    __builtin_amdgcn_sched_group_barrier(0x008, 32, 0);
  }
  wait_vmcnt<0>();  // the redundant pieces of the last iteration have landed
  __builtin_amdgcn_s_barrier();  // all fragment reads done, no DMA in flight: LDS is free for the epilogue
#ifdef CODETR_GEMM_STAMPS
  if (threadIdx.x == 0) st1 = __builtin_amdgcn_s_memtime();
#endif

  // epilogue (the output rule of gemm_epilogue.h) in two 64-row halves per wave through its private staging region
  // (64 rows x 144 B), as in linear_body
  constexpr int kPitch = kStagePitch;
  unsigned char* stage = lds + wave * (64 * kPitch);
  const int srow = lane >> 3, schunk = lane & 7;
  const int n = n0 + wn * 64 + schunk * 8;
  unsigned char* ytile = reinterpret_cast<unsigned char*>(Y) + ((size_t)m0 * N + n0) * 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = epi_act<ACT, HAS_RES>(acc[i][h * 4 + j][r]);
        *reinterpret_cast<s16x4*>(stage + (j * 16 + frow) * kPitch + (i * 16 + ncol) * 2) = T::pack4(v);
      }
    __builtin_amdgcn_wave_barrier();
    // residual rows of this half, all requested before the first use (one exposed latency instead of eight)
    s16x8 rres[8];
    if (HAS_RES) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        int m = m0 + wm * 128 + h * 64 + it * 8 + srow;
        m = m < M ? m : M - 1;
        rres[it] = *reinterpret_cast<const s16x8*>(R + (size_t)m * N + epi_residual_col(n, N));
      }
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int ml = it * 8 + srow;
      const int m = m0 + wm * 128 + h * 64 + ml;
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
        if (HAS_RES) {
          const s16x8 rr = rres[it];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = (short)epi_residual<T, ACT>((unsigned short)v[e], (unsigned short)rr[e]);
        }
        // uniform 64-bit tile base (SGPRs) + 32-bit lane offset: the store carries half the address bytes
        const unsigned loff = ((unsigned)(wm * 128 + h * 64 + ml) * (unsigned)N + (unsigned)(wn * 64 + schunk * 8)) * 2u;
        *reinterpret_cast<s16x8*>(ytile + loff) = v;
      }
    }
    __builtin_amdgcn_wave_barrier();  // the region is rewritten by the second half
  }
#ifdef CODETR_GEMM_STAMPS
  if (threadIdx.x == 0 && g_stamps) {
    st2 = __builtin_amdgcn_s_memtime();   // all stores of wave 0 issued (not completed)
    wait_vmcnt<0>();
    const unsigned long long st3 = __builtin_amdgcn_s_memtime();   // ... and completed
    unsigned long long* o = g_stamps + 8 * (size_t)blockIdx.x;
    o[0] = st0; o[1] = st1; o[2] = st2; o[3] = st3; o[4] = rt0; o[5] = __builtin_amdgcn_s_memrealtime();
    o[6] = wait_dma; o[7] = wait_bar;
  }
#endif
}

template <class T, int ACT>
int launch_big(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y, const void* mask,
               int M, int N, int K) {
  const int tiles_m = (M + 255) / 256, tiles_n = (N + 255) / 256;
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(512);
  const Operands o(X, W, bias, R, Y, mask);
  // scalar-base LDS-DMA for problems of more than one column tile (-1 ... -2.5 %; a single column tile -- N = 192 --
  // measured 6 % slower with it and keeps the pointer form)
  const bool sdma = tiles_n > 1;
  dispatch_bias_res(bias, R, [&](auto hb, auto hr) {
    auto* kernel = sdma ? linear_256_kernel<T, ACT, hb(), hr(), true> : linear_256_kernel<T, ACT, hb(), hr(), false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, o.x, o.w, o.b, o.r, o.y, o.mk, M, N, K, tiles_n);
  });
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

// the 256-tile kernel: K >= 256 (K = 256 layers whose N fills 256-wide tiles -- value / output
// projections, enc_output -- measured 5-15 % faster here than on the X-stationary kernel), see pick_kernel in gemm_f16.hip
bool gemm_route::big_applicable(int64_t M, int64_t N, int64_t K, int hm_hd) {
  if (hm_hd != 0 || K < 256 || K % 64 != 0 || N % 8 != 0) return false;
  const int64_t tn = (N + 255) / 256, tm = (M + 255) / 256;
  // at least ~0.8 tiles per CU (200 measured better than 512 for the single-image shapes: Swin stage-2 fc1 78 -> 67 us,
  // stage-3 qkv 58 -> 46 us), and little of the 256-wide tile wasted: >= 87.5 % of the tile columns real,
  // or >= 75 % when one column tile covers N (X is then read exactly once: Swin stage-0 fc2, N = 192, 806 -> 678 us)
  return tm * tn >= 200 && (N * 8 >= tn * 256 * 7 || (tn == 1 && N * 4 >= 256 * 3));
}

int gemm_route::launch_tile256(hipStream_t st, bool bf16, const void* X, const void* W, const void* bias, const void* R,
                               void* Y, const void* mask, int M, int N, int K, int act) {
  return dispatch_elem(bf16, [&](auto t) {
    return dispatch_act(act, [&](auto a) { return launch_big<decltype(t), a()>(st, X, W, bias, R, Y, mask, M, N, K); });
  });
}
