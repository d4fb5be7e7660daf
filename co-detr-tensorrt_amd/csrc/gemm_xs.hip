// The X-stationary kernel of the fused linear layer (gemm_f16.hip is the front door and says what the layer is):
// Y[M,N] = act(X[M,K] . W[N,K]^T + bias[N]) (+ R[M,N]), fp16 / bf16 storage, fp32 accumulation on the matrix cores,
// for K = 64, 192, 256 and 128 <= N <= 1536 (xs_applicable below), and the forms only this kernel has: LayerNorm of the
// input rows (codetr_linear_ln_*), x + x2 on the way in (codetr_linear_xadd_*), fp16 output of bf16 operands
// (codetr_linear_bf16_f16out) and the encoder's two projections as one launch (codetr_encoder_projections*).
//
// X-stationary kernel for the short-K layers (K = 192, 256, 384: Swin stages 0-1 and every 256-wide transformer
// layer -- a third of the model's GEMM time).  The 128-tile kernel (gemm_tile128.hip) re-reads each 128 x K activation tile from L2
// once per 128-column output tile and pays its fixed per-tile cost (first loads, staging, stores) N/128 times; with
// K this short the whole K extent of 32 rows fits a wave's registers.  So, as in the first product of
// ffn_fused.hip: a 256-thread workgroup owns 128 rows for ALL N; each wave loads its 32 rows of X once, as MFMA B
// fragments straight from global memory (KS k-steps x 2 m-tiles), and keeps them; W streams through a 2-stage LDS
// ring in chunks of 32 output columns (32 x K, LDS-DMA, XOR-swizzled on the source address), D[n][m] = W . X^T, so
// a lane again owns 4 consecutive n of one row.  Per chunk: bias from LDS into the accumulator init, 16*KS/8 MFMAs
// per wave, activation, fp16 image of the wave's 32 x 32 piece in its private LDS region, row-wise read-back,
// residual (requested before the MFMAs) / row mask, 16-B stores.  X is read from HBM exactly once, Y written once,
// W (<= 1.2 MB) comes from L2.
#include "gemm_route.h"
#include "gemm_tile.h"

namespace {

// diagnostic builds only (tools/micro/build_variant.sh ... "-DCODETR_XS_ABL=mask", WRONG results by construction): 1 = no output
// stores, 2 = no MFMAs, 4 = no W chunk staging inside the loop, 8 = no wait / barrier per chunk, 16 = no X / X2 loads
#ifndef CODETR_XS_ABL
#define CODETR_XS_ABL 0
#endif
#ifdef CODETR_XS_STAMPS   // diagnostic build only (tools/micro/xs_stamps.hip): where wave 0 of every workgroup spends its cycles
__device__ unsigned long long* g_xs_stamps = nullptr;
#define XS_STAMP(i) xs_t[i] = __builtin_readcyclecounter()
#else
#define XS_STAMP(i)
#endif
//
// SPLIT (the encoder's two projections of one token row as ONE launch -- reference multi_scale_deformable_attention.py:161-179:
// value_proj(value) and sampling_offsets | attention_weights (query + query_pos), where value IS query): W holds N1 rows
// applied to X and N - N1 rows applied to X + X2; the first N1 columns go to Y (type OT, row mask, optional head-major
// layout), the others to Y2 (type T, row-major, N - N1 columns).  The kept fragments become X + X2 at chunk N1 / 32: X and
// X2 are each read once for both products (two launches read X twice: 419 MB of 2.5 GB at four 1920x1280 images).
// POSGEN (SPLIT only, round 6): X2 is the encoder's sine positional encoding + level embedding -- a pure function of the
// token's (level, y, x) and of the running sums of the padding mask (reference positional_encoding.py:58-93 +
// transformer.py:508-519, csrc/sine_pos.hip) -- and is GENERATED here instead of read: the lane re-derives its row's two
// normalised coordinates from the running sums (8 bytes per token instead of the row's 512) and evaluates its 64 channels
// with the SAME fp32 operations, in the same order, as sine_pos_kernel, so the operand x + pos is bit-identical to the one
// read from the tensor that kernel writes.  Saves the 64 KiB of pos rows per 128-row tile and the exposed wait for them at
// the start of the second product.
struct XsPosGen {
  const float* ycum[5];                 // per level: running sums of the not-mask along y, [B, H_l, W_l] fp32
  const float* xcum[5];                 // ... along x
  const unsigned short* level_embed;    // [L, 256] in the operands' type (nullptr: none)
  int H[5], W[5], start[5];             // level l holds tokens start[l] .. start[l] + H W - 1 of an image's S
  int L, S;
  float log2_temperature, scale, eps, offset;
  int normalize;
};

template <class T, int KS, int ACT, bool HAS_RES, class OT = T, bool SPLIT = false, bool POSGEN = false>   // OT: storage type of Y (bf16 operands -> fp16 output: the
__global__ __launch_bounds__(256) void linear_xs_kernel(const unsigned short* __restrict__ X,   // encoder MSDA's value map)
                                                        const unsigned short* __restrict__ X2,
                                                        const unsigned short* __restrict__ LNG,
                                                        const unsigned short* __restrict__ LNB, float ln_eps,
                                                        const unsigned short* __restrict__ W,
                                                        const unsigned short* __restrict__ bias,
                                                        const unsigned short* __restrict__ R,
                                                        unsigned short* __restrict__ Y,
                                                        const unsigned char* __restrict__ row_mask, int M, int N, int hm_rows,
                                                        int hm_hd, unsigned short* __restrict__ Y2 = nullptr, int N1 = 0,
                                                        const XsPosGen pg = XsPosGen()) {
  constexpr int K = KS * 32, CH = K / 8;          // 16-byte chunks per row
  constexpr int CN = 32;                          // output columns per W chunk
  constexpr int kChunkBytes = CN * K * 2;         // 12 / 16 / 24 KiB
  constexpr int kPieces = kChunkBytes / 4096;     // LDS-DMA instructions per thread per chunk (3 / 4 / 6)
  constexpr int kXsPitch = 2 * CN * 2 + 16;       // staged output row: two chunks side by side, 128 B + 16
  constexpr int kStage = 4 * 32 * kXsPitch;       // 18 KiB: 4 waves x 32 rows
  constexpr int kMaxBias = 1568;
  constexpr int SWZ = (CH % 16 == 0) ? 15 : 7;    // XOR mask that keeps a swizzled chunk inside its row
  constexpr int kRing = 3;                        // W chunks in flight: c (being multiplied), c + 1, c + 2
  constexpr int kLeBytes = POSGEN ? 5 * K * 2 : 0;   // the level embeddings (POSGEN)
  __shared__ __attribute__((aligned(16))) unsigned char lds[kRing * kChunkBytes + kStage + kMaxBias * 2 + kLeBytes];
  unsigned char* stage_base = lds + kRing * kChunkBytes;
  unsigned short* sBias = reinterpret_cast<unsigned short*>(lds + kRing * kChunkBytes + kStage);
  unsigned short* sLe = sBias + kMaxBias;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, grp = lane >> 4;
  const int m0 = (int)xcd_tile(blockIdx.x, gridDim.x) * 128 + wave * 32;
  const int nchunks = (N + CN - 1) / CN;
#ifdef CODETR_XS_STAMPS
  unsigned long long xs_t[8], xs_acc[6] = {0, 0, 0, 0, 0, 0};
  const unsigned long long xs_start = __builtin_readcyclecounter(), xs_rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int Ny = SPLIT ? N1 : N;                  // columns of Y (SPLIT: the others are Y2's)
  const int c1 = SPLIT ? N1 / CN : 0;             // first chunk of the second product

  // LDS-DMA of one W chunk (32 rows x K, kPieces pieces of 4 KiB): piece q covers rows (q * 256 + tid) / CH.  Inline
  // assembly with a wave-uniform base and a per-thread byte offset (see lds_dma16s): no vector arithmetic per piece but
  // the row clamp of a ragged last chunk, and the compiler keeps counting its ds_read waits.
  unsigned piece_row[kPieces], piece_off[kPieces];
#pragma unroll
  for (int q = 0; q < kPieces; ++q) {
    const int u = q * 256 + tid;
    const int r = u / CH, pos = u % CH;
    piece_row[q] = (unsigned)r;
    piece_off[q] = (unsigned)((pos ^ (r & SWZ)) * 16);
  }
  const unsigned char* Wb = reinterpret_cast<const unsigned char*>(W);
  auto stage_chunk = [&](int c, unsigned char* dst) {
    const unsigned rmax = (unsigned)(N - 1 - c * CN);  // ragged last chunk: re-read the last row, its columns are never stored
#pragma unroll
    for (int q = 0; q < kPieces; ++q) {
      const unsigned r = piece_row[q] < rmax ? piece_row[q] : rmax;
      lds_dma16(Wb + (size_t)c * kChunkBytes, r * (unsigned)(K * 2) + piece_off[q], dst + (q * 256 + wave * 64) * 16);
    }
  };
  stage_chunk(0, lds);
  stage_chunk(nchunks > 1 ? 1 : 0, lds + kChunkBytes);   // (a single chunk: a second fetch nobody reads keeps the counts uniform)

  // this wave's 32 rows of X, B-operand fragments: lane (j = l15, g = grp) holds X[m][32*ks + 8g .. +7]
  typename T::frag xf[2][KS];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    int m = m0 + mt * 16 + l15;
    m = m < M ? m : M - 1;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (CODETR_XS_ABL & 16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[mt][ks][e] = (typename T::elem)(float)(m + ks);
        continue;
      }
      xf[mt][ks] = *reinterpret_cast<const typename T::frag*>(X + (size_t)m * K + ks * 32 + grp * 8);
    }
    // optional second input, added element-wise on the way in (x + x2 rounded to T, the fp16 / bf16 add the host
    // would otherwise run as its own kernel: `query + query_pos` in front of the offsets | logits projection)
    if (X2 && !SPLIT && !(CODETR_XS_ABL & 16)) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const typename T::frag p = *reinterpret_cast<const typename T::frag*>(X2 + (size_t)m * K + ks * 32 + grp * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[mt][ks][e] = (typename T::elem)((float)xf[mt][ks][e] + (float)p[e]);
      }
    }
    // optional LayerNorm of the input rows (the whole row is in this wave: K values in the four lanes l15 + 16 g), fp32
    // two-pass statistics, result rounded to T = the operand a separate LayerNorm kernel would have written; used
    // where nothing else reads that normalised tensor (Swin's pre-norm blocks: norm1 -> qkv, norm2 -> fc1)
    if (LNG) {
      float sm = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) sm += (float)xf[mt][ks][e];
      sm += __shfl_xor(sm, 16, 64);
      sm += __shfl_xor(sm, 32, 64);
      const float mean = sm * (1.0f / K);
      float q = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = (float)xf[mt][ks][e] - mean;
          q = fmaf(d, d, q);
        }
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      const float rstd = rsqrtf(q * (1.0f / K) + ln_eps);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const typename T::frag gw = *reinterpret_cast<const typename T::frag*>(LNG + ks * 32 + grp * 8);
        const typename T::frag gb = *reinterpret_cast<const typename T::frag*>(LNB + ks * 32 + grp * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          xf[mt][ks][e] = (typename T::elem)fmaf(((float)xf[mt][ks][e] - mean) * rstd, (float)gw[e], (float)gb[e]);
      }
    }
  }
  // POSGEN: this lane's two rows -> level, normalised coordinates (the running sums are requested here, next to the rows)
  float pg_ey[2] = {0.f, 0.f}, pg_ex[2] = {0.f, 0.f};
  int pg_lv[2] = {0, 0};
  if constexpr (POSGEN) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      int m = m0 + mt * 16 + l15;
      m = m < M ? m : M - 1;
      const int b = m / pg.S, tok = m - b * pg.S;
      int l = 0;
#pragma unroll
      for (int k = 1; k < 5; ++k) l += (k < pg.L && tok >= pg.start[k]) ? 1 : 0;
      int Hl = pg.H[0], Wl = pg.W[0], st = pg.start[0];
      const float* yc = pg.ycum[0];
      const float* xc = pg.xcum[0];
#pragma unroll
      for (int k = 1; k < 5; ++k) {
        const bool me = l == k;
        Hl = me ? pg.H[k] : Hl;
        Wl = me ? pg.W[k] : Wl;
        st = me ? pg.start[k] : st;
        yc = me ? pg.ycum[k] : yc;
        xc = me ? pg.xcum[k] : xc;
      }
      const int r = tok - st, y = r / Wl, x = r - y * Wl;
      const int64_t base = (int64_t)b * Hl * Wl;
      float ey = yc[base + r], ex = xc[base + r];
      if (pg.normalize) {   // exactly sine_pos_kernel's expression
        const float ly = yc[base + (int64_t)(Hl - 1) * Wl + x], lx = xc[base + (int64_t)y * Wl + (Wl - 1)];
        ey = (ey + pg.offset) / (ly + pg.eps) * pg.scale;
        ex = (ex + pg.offset) / (lx + pg.eps) * pg.scale;
      }
      pg_ey[mt] = ey;
      pg_ex[mt] = ex;
      pg_lv[mt] = l;
    }
    if (pg.level_embed)
      for (int i = tid; i < pg.L * K / 8; i += 256)
        *reinterpret_cast<s16x8*>(sLe + i * 8) = *reinterpret_cast<const s16x8*>(pg.level_embed + i * 8);
  }
  if (bias) {
    for (int i = tid; i < N / 8; i += 256)
      *reinterpret_cast<s16x8*>(sBias + i * 8) = *reinterpret_cast<const s16x8*>(bias + i * 8);
  }
  // the row states of the lane's four output rows (m0 + 8 it + (lane >> 3)), fetched ONCE here: read inside the chunk loop
  // they sat behind the LDS-DMA pieces in flight (vector memory returns in order) -- + 16-19 % on the decoder's value
  // projection (924 -> 1 100 us at 4 images)
  unsigned row_states = 0;
  if (row_mask) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int m = m0 + it * 8 + (lane >> 3);
      row_states |= (m < M ? (unsigned)row_mask[m] : 0u) << (8 * it);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  unsigned char* my_stage = stage_base + wave * (32 * kXsPitch);
  // Outputs leave two chunks at a time: 64 columns = 128 contiguous bytes per row, i.e. whole cache lines (a single
  // 32-column chunk would write half lines and leave the merge to the L2).  Read-back of a pair: 8 rows x 8 chunks of
  // 16 B per step, 4 steps.
  const int srow = lane >> 3, schunk = lane & 7;
  s16x8 rr[4];
  // residual rows of the pair that starts at column np (requested one chunk before they are added)
  auto load_residual = [&](int np) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      int m = m0 + it * 8 + srow;
      m = m < M ? m : M - 1;
      const int n = epi_residual_col(np + schunk * 8, N);
      rr[it] = *reinterpret_cast<const s16x8*>(R + (size_t)m * N + n);
    }
  };
  // the staged pair that starts at column np: + residual / row mask, 16-byte stores of whole 128-byte row segments
  auto flush_pair = [&](int np) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int ml = it * 8 + srow;
      const int m = m0 + ml;
      const int n = np + schunk * 8;
      s16x8 v = *reinterpret_cast<const s16x8*>(my_stage + ml * kXsPitch + schunk * 16);
      if (SPLIT && np >= N1) {   // (N1 % 64 == 0: a pair belongs to one of the two outputs)
        if (m < M && n < N) *reinterpret_cast<s16x8*>(Y2 + (size_t)m * (N - N1) + (n - N1)) = v;
        continue;
      }
      if (m < M && n < Ny) {  // N % 8 == 0: a chunk of 8 columns is inside or outside as a whole
        if (row_mask)
          epi_row_state<T, OT, ACT, HAS_RES>(v, (unsigned char)((row_states >> (8 * it)) & 0xffu), bias != nullptr, sBias, n);
        if (HAS_RES) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = (short)epi_residual<T, ACT>((unsigned short)v[e], (unsigned short)rr[it][e]);
        }
        size_t off = (size_t)m * Ny + n;
        if (hm_hd > 0) off = epi_head_major(m, n, Ny, hm_rows, hm_hd);
        if (!(CODETR_XS_ABL & 1) || v[0] == 0x1234) *reinterpret_cast<s16x8*>(Y + off) = v;
      }
    }
    __builtin_amdgcn_wave_barrier();  // the staging region is rewritten by the next pair
  };
  // Schedule (vmcnt counts LDS-DMA pieces, loads and stores in issue order).  Chunk c:
  //   wait until W[c] landed: everything but the kPieces pieces of W[c+1], the youngest operations, is complete --
  //     including the stores of the pair flushed a whole chunk earlier, so nobody ever waits for a store just issued
  //     (the 2-stage form of this loop waited `vmcnt(0)` right behind its own stores: 2.8 us per chunk for 0.25 us of
  //     MFMAs); barrier: W[c] is visible, everyone is done with W[c-1]
  //   even c >= 2: flush the pair (c-2, c-1) staged by the previous two chunks; odd c: request that pair's residual rows
  //   issue W[c+2] into the stage W[c-1] used
  //   32 x 32 outputs per wave: MFMAs, activation, fp16 image into the wave's staging region
  int slot = 0;  // ring slot of W[c]
#ifdef CODETR_XS_STAMPS
  const unsigned long long xs_loop = __builtin_readcyclecounter();
#endif
  for (int c = 0; c < nchunks; ++c) {
    XS_STAMP(0);
    if (!(CODETR_XS_ABL & 8)) wait_vmcnt<kPieces>();
    XS_STAMP(1);
    if (!(CODETR_XS_ABL & 8)) __builtin_amdgcn_s_barrier();
    XS_STAMP(2);
    const int n0 = c * CN;
    if (!(c & 1)) {
      if (c >= 2) flush_pair((c - 2) * CN);
    } else if (HAS_RES) {
      load_residual((c - 1) * CN);
    }
    XS_STAMP(3);
    {
      const int c2 = c + 2 < nchunks ? c + 2 : nchunks - 1;  // (past the end: a fetch nobody reads, same counts)
      const int s2 = slot == 0 ? 2 : slot - 1;               // the slot W[c-1] used
      if (!(CODETR_XS_ABL & 4)) stage_chunk(c2, lds + s2 * kChunkBytes);
    }
    XS_STAMP(4);
    if (SPLIT && c == c1) {
      // the second product's operand: x + x2 rounded to T (exactly the separate add); its loads are the youngest vector
      // memory operations and are waited for here, so the counted wait of the next chunk sees the W pieces only
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        int m = m0 + mt * 16 + l15;
        m = m < M ? m : M - 1;
        if constexpr (POSGEN) {
          // lane (row l15, group g) holds channels 32 ks + 8 g .. + 7 = 16-byte chunk c = 4 ks + g of the row: ks < KS / 2 the y
          // half, the others the x half; chunk (c mod 16) covers frequencies 4 (c mod 16) .. + 3 (channel 2f: sin, 2f + 1: cos).
          // One fragment at a time, added as it is made (eight live fragments cost the second workgroup of the CU its registers).
          static_assert(!POSGEN || KS == 8, "256 channels");
          constexpr int num_feats = K / 2;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            typename T::frag pfk;
            const float e_ = ks >= KS / 2 ? pg_ex[mt] : pg_ey[mt];
            const int ch0 = (4 * (ks & 3) + grp) * 8;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const int f = (ch0 >> 1) + p;
              const float inv = __builtin_amdgcn_exp2f(-pg.log2_temperature * (2.0f * (float)f / (float)num_feats));
              const float rev = e_ * inv * 0.15915494309189535f;
              pfk[2 * p] = (typename T::elem)__builtin_amdgcn_sinf(rev);
              pfk[2 * p + 1] = (typename T::elem)__builtin_amdgcn_cosf(rev);
            }
            if (pg.level_embed) {
              const typename T::frag le = *reinterpret_cast<const typename T::frag*>(sLe + pg_lv[mt] * K + (4 * ks + grp) * 8);
#pragma unroll
              for (int k = 0; k < 8; ++k) pfk[k] = (typename T::elem)((float)pfk[k] + (float)le[k]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) xf[mt][ks][e] = (typename T::elem)((float)xf[mt][ks][e] + (float)pfk[e]);
            asm volatile("" : "+v"(pg_ey[mt]), "+v"(pg_ex[mt]));   // (keeps the frequency factors from being hoisted out of the loops)
          }
        } else {
          typename T::frag pf[KS];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            pf[ks] = *reinterpret_cast<const typename T::frag*>(X2 + (size_t)m * K + ks * 32 + grp * 8);
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) xf[mt][ks][e] = (typename T::elem)((float)xf[mt][ks][e] + (float)pf[ks][e]);
        }
      }
    }
    const unsigned char* sW = lds + slot * kChunkBytes;
    slot = slot == 2 ? 0 : slot + 1;

    f32x4 acc[2][2];  // [n-tile][m-tile]
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
      if (bias) {
        const s16x4 bv = *reinterpret_cast<const s16x4*>(sBias + n0 + nt * 16 + grp * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) b4[r] = T::to_f32((unsigned short)bv[r]);
      }
      acc[nt][0] = b4;
      acc[nt][1] = b4;
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      typename T::frag a[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int row = nt * 16 + l15;
        const int chunk = (ks * 4 + grp) ^ (row & SWZ);
        a[nt] = *reinterpret_cast<const typename T::frag*>(sW + row * (K * 2) + chunk * 16);
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          if (CODETR_XS_ABL & 2) acc[nt][mt][0] += (float)a[nt][0] * (float)xf[mt][ks][0];
          else acc[nt][mt] = T::mfma(a[nt], xf[mt][ks], acc[nt][mt]);
        }
    }
    // ---- chunk epilogue: this wave's 32 rows x 32 columns into its half of the staged pair ----
#ifdef CODETR_XS_STAMPS
    asm volatile("" ::"v"(acc[1][1][3]) : "memory");
#endif
    XS_STAMP(5);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = epi_act<ACT, HAS_RES>(acc[nt][mt][r]);
        *reinterpret_cast<s16x4*>(my_stage + (mt * 16 + l15) * kXsPitch + ((c & 1) * CN + nt * 16 + grp * 4) * 2) =
            (SPLIT && c >= c1) ? T::pack4(v) : OT::pack4(v);
      }
#ifdef CODETR_XS_STAMPS
    asm volatile("" ::: "memory");
    XS_STAMP(6);
#pragma unroll
    for (int i = 0; i < 6; ++i) xs_acc[i] += xs_t[i + 1] - xs_t[i];
#endif
  }
  // the last pair (one chunk if nchunks is odd)
  {
    const int np = ((nchunks - 1) & ~1) * CN;
    if (HAS_RES && (nchunks & 1)) load_residual(np);   // (an even count requested it in the last chunk)
    flush_pair(np);
  }
  wait_vmcnt<0>();  // the redundant fetches of the last two iterations
#ifdef CODETR_XS_STAMPS
  if (threadIdx.x == 0 && g_xs_stamps) {
    unsigned long long* o = g_xs_stamps + 12 * (size_t)blockIdx.x;
#pragma unroll
    for (int i = 0; i < 6; ++i) o[i] = xs_acc[i];
    o[6] = xs_loop - xs_start;                       // prologue
    o[7] = __builtin_readcyclecounter() - xs_start;  // whole workgroup
    o[8] = xs_rt0;
    o[9] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

using gemm_route::xs_applicable;   // (the kernel's domain: defined behind this namespace)

template <class T, int KS, int ACT, class OT = T>
int launch_xs_res(hipStream_t st, const void* X, const void* W, const void* bias, const void* R, void* Y,
                  const void* mask, int M, int N, int hm_rows, int hm_hd, const void* X2 = nullptr,
                  const void* LNG = nullptr, const void* LNB = nullptr, float ln_eps = 0.f) {
  const dim3 grid((unsigned)((M + 127) / 128)), block(256);
  const Operands o(X, W, bias, R, Y, mask);
  if (R && std::is_same<T, OT>::value)
    hipLaunchKernelGGL((linear_xs_kernel<T, KS, ACT, true, T>), grid, block, 0, st, o.x, u16(X2), u16(LNG), u16(LNB), ln_eps, o.w, o.b, o.r, o.y, o.mk, M, N, hm_rows, hm_hd);
  else if (R) return CODETR_E_UNSUPPORTED;   // (a residual is added in the operands' type)
  else hipLaunchKernelGGL((linear_xs_kernel<T, KS, ACT, false, OT>), grid, block, 0, st, o.x, u16(X2), u16(LNG), u16(LNB), ln_eps, o.w, o.b, o.r, o.y, o.mk, M, N, hm_rows, hm_hd);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

// x + x2 folded into the X-stationary kernel's operand load (act 0, no residual / mask): only where that kernel applies
template <class T>
int launch_xadd(hipStream_t st, const void* X, const void* X2, const void* W, const void* bias, void* Y, int64_t M,
                int64_t N, int64_t K) {
  if (!X || !X2 || !W || !Y || M <= 0 || N <= 0 || K <= 0) return CODETR_E_BADARG;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (!xs_applicable(M, N, K, 0) || K == 64 || !aligned16(Y, X, X2, W)) return CODETR_E_UNSUPPORTED;
  return dispatch_ks(K, [&](auto ks) {
    return launch_xs_res<T, ks(), 0>(st, X, W, bias, nullptr, Y, nullptr, (int)M, (int)N, 0, 0, X2);
  });
}

// LayerNorm of the input rows folded into the X-stationary kernel (no residual / mask): only where that kernel applies
template <class T>
int launch_ln(hipStream_t st, const void* X, const void* G, const void* Bt, float eps, const void* W, const void* bias,
              void* Y, int64_t M, int64_t N, int64_t K, int act) {
  if (!X || !G || !Bt || !W || !Y || M <= 0 || N <= 0 || K <= 0 || act < 0 || act > 2) return CODETR_E_BADARG;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (!xs_applicable(M, N, K, 0) || K == 64 || !aligned16(Y, X, G, Bt, W)) return CODETR_E_UNSUPPORTED;
  return dispatch_act(act, [&](auto a) {
    return dispatch_ks(K, [&](auto ks) {
      return launch_xs_res<T, ks(), a()>(st, X, W, bias, nullptr, Y, nullptr, (int)M, (int)N, 0, 0, nullptr, G, Bt, eps);
    });
  });
}

// the argument checks of the two SPLIT launchers below; 0 or a CODETR_E_ code.  second: the operand of the second product
// that must be 16-byte aligned (X2, or the level embedding); own: the code of the caller's own range checks, which rank
// behind the null / sign checks and ahead of everything else
int split_check(const void* X, const void* second, const void* W, const void* bias, const void* Y, const void* Y2, int64_t M,
                int64_t N1, int64_t N2, int64_t K, int64_t hm_rows, int hm_hd, int own = 0) {
  if (!X || !W || !Y || !Y2 || M <= 0 || N1 <= 0 || N2 <= 0 || K <= 0) return CODETR_E_BADARG;
  if (own) return own;
  if (M > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (!aligned16(X, second, W, Y, Y2, bias)) return CODETR_E_BADARG;
  if (hm_hd != 0 || hm_rows != 0) {
    if (hm_hd <= 0 || hm_rows <= 0 || hm_hd % 8 != 0 || N1 % hm_hd != 0 || M % hm_rows != 0) return CODETR_E_UNSUPPORTED;
  }
  if (K != 256 || N1 % 64 != 0 || N2 % 8 != 0 || N1 + N2 > 1536 || M < 128 * 256) return CODETR_E_UNSUPPORTED;
  return 0;
}

// the encoder's two projections as one launch of the X-stationary kernel (SPLIT form): K = 256 only
template <class T, class OT>
int launch_split(hipStream_t st, const void* X, const void* X2, const void* W, const void* bias, const void* mask, void* Y,
                 void* Y2, int64_t M, int64_t N1, int64_t N2, int64_t K, int64_t hm_rows, int hm_hd) {
  if (!X2) return CODETR_E_BADARG;
  if (const int rc = split_check(X, X2, W, bias, Y, Y2, M, N1, N2, K, hm_rows, hm_hd)) return rc;
  const dim3 grid((unsigned)((M + 127) / 128)), block(256);
  const Operands o(X, W, bias, nullptr, Y, mask);
  hipLaunchKernelGGL((linear_xs_kernel<T, 8, 0, false, OT, true>), grid, block, 0, st, o.x, u16(X2), nullptr, nullptr, 0.f,
                     o.w, o.b, nullptr, o.y, o.mk, (int)M, (int)(N1 + N2), (int)hm_rows, hm_hd,
                     static_cast<unsigned short*>(Y2), (int)N1);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

// ... with the positional operand generated in the kernel (POSGEN): same checks, plus the pyramid
template <class T, class OT>
int launch_split_pos(hipStream_t st, const void* X, const float* const* ycum, const float* const* xcum,
                     const int64_t* shapes, int L, const void* level_embed, float temperature, float scale, float eps,
                     float offset, int normalize, const void* W, const void* bias, const void* mask, void* Y, void* Y2,
                     int64_t M, int64_t S, int64_t N1, int64_t N2, int64_t K, int64_t hm_rows, int hm_hd) {
  if (!ycum || !xcum || !shapes || S <= 0 || L <= 0 || !(temperature > 0.f)) return CODETR_E_BADARG;
  const int own = L > 5 ? CODETR_E_UNSUPPORTED : M % S != 0 ? CODETR_E_BADARG : 0;
  if (const int rc = split_check(X, level_embed, W, bias, Y, Y2, M, N1, N2, K, hm_rows, hm_hd, own)) return rc;
  XsPosGen pg;
  int64_t sum = 0;
  for (int l = 0; l < 5; ++l) {
    pg.ycum[l] = l < L ? ycum[l] : nullptr;
    pg.xcum[l] = l < L ? xcum[l] : nullptr;
    const int64_t h = l < L ? shapes[2 * l] : 1, w = l < L ? shapes[2 * l + 1] : 1;
    if (l < L && (!ycum[l] || !xcum[l] || h <= 0 || w <= 0 || h > 32767 || w > 32767)) return CODETR_E_BADARG;
    pg.H[l] = (int)h;
    pg.W[l] = (int)w;
    pg.start[l] = l < L ? (int)sum : 0x7fffffff;
    if (l < L) sum += h * w;
  }
  if (sum != S) return CODETR_E_BADARG;
  pg.level_embed = u16(level_embed);
  pg.L = L;
  pg.S = (int)S;
  pg.log2_temperature = log2f(temperature);
  pg.scale = scale;
  pg.eps = eps;
  pg.offset = offset;
  pg.normalize = normalize;
  const dim3 grid((unsigned)((M + 127) / 128)), block(256);
  const Operands o(X, W, bias, nullptr, Y, mask);
  hipLaunchKernelGGL((linear_xs_kernel<T, 8, 0, false, OT, true, true>), grid, block, 0, st, o.x, nullptr, nullptr, nullptr,
                     0.f, o.w, o.b, nullptr, o.y, o.mk, (int)M, (int)(N1 + N2), (int)hm_rows, hm_hd,
                     static_cast<unsigned short*>(Y2), (int)N1, pg);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

// The short-K kernel serves f16 / bf16, K in {192, 256}, N % 8 == 0 (16-byte row chunks), 128 <= N <= 1536 (bias in
// LDS; narrower outputs measured equal or slower), at least one workgroup per CU (below that the tiled kernel's
// N-parallelism wins); column-block-major output only for blocks of a multiple of 64 columns (a stored chunk pair
// must not straddle blocks: the six decoder value projections as one N = 1536 GEMM, not the 32-wide MSDA heads).  K = 384 (Swin stage 1) fits the registers but measured 20-30 % slower
// than the tiled kernel (2 workgroups per CU, 48 MFMAs per barrier) and stays there.
bool gemm_route::xs_applicable(int64_t M, int64_t N, int64_t K, int hm_hd) {
  // (K = 64: the patch-embedding GEMM of the Swin stem, act 0 / no residual only)
  return (K == 192 || K == 256 || K == 64) && N % 8 == 0 && N >= 128 && N <= 1536 && M >= 128 * 256 && hm_hd % 8 == 0;
}

// behind codetr_linear_*: K = 64 (the patch embedding) is served without activation or residual, as pick_kernel requires
int gemm_route::launch_xs(hipStream_t st, bool bf16, const void* X, const void* W, const void* bias, const void* R, void* Y,
                          const void* mask, int M, int N, int K, int act, int hm_rows, int hm_hd) {
  return dispatch_elem(bf16, [&](auto t) {
    using T = decltype(t);
    if (K == 64) return launch_xs_res<T, 2, 0>(st, X, W, bias, nullptr, Y, mask, M, N, hm_rows, hm_hd);
    return dispatch_ks(K, [&](auto ks) {
      return dispatch_act(act, [&](auto a) { return launch_xs_res<T, ks(), a()>(st, X, W, bias, R, Y, mask, M, N, hm_rows, hm_hd); });
    });
  });
}

extern "C" {

int codetr_encoder_projections_posgen_f16(void* stream, const void* x_dev, const float* ycum0, const float* ycum1,
                                          const float* ycum2, const float* ycum3, const float* ycum4, const float* xcum0,
                                          const float* xcum1, const float* xcum2, const float* xcum3, const float* xcum4,
                                          const int64_t* level_shapes_host, int num_levels, const void* level_embed_dev,
                                          float temperature, float scale, float eps, float offset, int normalize,
                                          const void* w_dev, const void* bias_dev, const void* row_mask_dev, void* value_dev,
                                          void* packed_dev, int64_t M, int64_t S, int64_t N_value, int64_t N_packed, int64_t K,
                                          int64_t hm_rows, int hm_head_dim) {
  const float* yc[5] = {ycum0, ycum1, ycum2, ycum3, ycum4};
  const float* xc[5] = {xcum0, xcum1, xcum2, xcum3, xcum4};
  return launch_split_pos<HalfT, HalfT>(static_cast<hipStream_t>(stream), x_dev, yc, xc, level_shapes_host, num_levels,
                                        level_embed_dev, temperature, scale, eps, offset, normalize, w_dev, bias_dev, row_mask_dev,
                                        value_dev, packed_dev, M, S, N_value, N_packed, K, hm_rows, hm_head_dim);
}

int codetr_encoder_projections_posgen_bf16(void* stream, const void* x_dev, const float* ycum0, const float* ycum1,
                                          const float* ycum2, const float* ycum3, const float* ycum4, const float* xcum0,
                                          const float* xcum1, const float* xcum2, const float* xcum3, const float* xcum4,
                                          const int64_t* level_shapes_host, int num_levels, const void* level_embed_dev,
                                          float temperature, float scale, float eps, float offset, int normalize,
                                          const void* w_dev, const void* bias_dev, const void* row_mask_dev, void* value_f16_dev,
                                          void* packed_dev, int64_t M, int64_t S, int64_t N_value, int64_t N_packed, int64_t K,
                                          int64_t hm_rows, int hm_head_dim) {
  const float* yc[5] = {ycum0, ycum1, ycum2, ycum3, ycum4};
  const float* xc[5] = {xcum0, xcum1, xcum2, xcum3, xcum4};
  return launch_split_pos<BFloatT, HalfT>(static_cast<hipStream_t>(stream), x_dev, yc, xc, level_shapes_host, num_levels,
                                        level_embed_dev, temperature, scale, eps, offset, normalize, w_dev, bias_dev, row_mask_dev,
                                        value_f16_dev, packed_dev, M, S, N_value, N_packed, K, hm_rows, hm_head_dim);
}

int codetr_encoder_projections_f16(void* stream, const void* x_dev, const void* pos_dev, const void* w_dev,
                                   const void* bias_dev, const void* row_mask_dev, void* value_dev, void* packed_dev,
                                   int64_t M, int64_t N_value, int64_t N_packed, int64_t K, int64_t hm_rows, int hm_head_dim) {
  return launch_split<HalfT, HalfT>(static_cast<hipStream_t>(stream), x_dev, pos_dev, w_dev, bias_dev, row_mask_dev,
                                    value_dev, packed_dev, M, N_value, N_packed, K, hm_rows, hm_head_dim);
}

int codetr_encoder_projections_bf16(void* stream, const void* x_dev, const void* pos_dev, const void* w_dev,
                                    const void* bias_dev, const void* row_mask_dev, void* value_f16_dev, void* packed_dev,
                                    int64_t M, int64_t N_value, int64_t N_packed, int64_t K, int64_t hm_rows,
                                    int hm_head_dim) {
  return launch_split<BFloatT, HalfT>(static_cast<hipStream_t>(stream), x_dev, pos_dev, w_dev, bias_dev, row_mask_dev,
                                      value_f16_dev, packed_dev, M, N_value, N_packed, K, hm_rows, hm_head_dim);
}

int codetr_linear_ln_f16(void* stream, const void* x_dev, const void* ln_gamma_dev, const void* ln_beta_dev, float ln_eps,
                         const void* w_dev, const void* bias_dev, void* y_dev, int64_t M, int64_t N, int64_t K, int act) {
  return launch_ln<HalfT>(static_cast<hipStream_t>(stream), x_dev, ln_gamma_dev, ln_beta_dev, ln_eps, w_dev, bias_dev,
                          y_dev, M, N, K, act);
}

int codetr_linear_ln_bf16(void* stream, const void* x_dev, const void* ln_gamma_dev, const void* ln_beta_dev, float ln_eps,
                          const void* w_dev, const void* bias_dev, void* y_dev, int64_t M, int64_t N, int64_t K, int act) {
  return launch_ln<BFloatT>(static_cast<hipStream_t>(stream), x_dev, ln_gamma_dev, ln_beta_dev, ln_eps, w_dev, bias_dev,
                            y_dev, M, N, K, act);
}

int codetr_linear_xadd_f16(void* stream, const void* x_dev, const void* x_add_dev, const void* w_dev,
                           const void* bias_dev, void* y_dev, int64_t M, int64_t N, int64_t K) {
  return launch_xadd<HalfT>(static_cast<hipStream_t>(stream), x_dev, x_add_dev, w_dev, bias_dev, y_dev, M, N, K);
}

int codetr_linear_xadd_bf16(void* stream, const void* x_dev, const void* x_add_dev, const void* w_dev,
                            const void* bias_dev, void* y_dev, int64_t M, int64_t N, int64_t K) {
  return launch_xadd<BFloatT>(static_cast<hipStream_t>(stream), x_dev, x_add_dev, w_dev, bias_dev, y_dev, M, N, K);
}

int codetr_linear_bf16_f16out(void* stream, const void* x_dev, const void* w_dev, const void* bias_dev,
                              const void* row_mask_dev, void* y_dev, int64_t M, int64_t N, int64_t K, int64_t hm_rows,
                              int hm_head_dim) {
  if (!x_dev || !w_dev || !y_dev || M <= 0 || N <= 0 || K <= 0) return CODETR_E_BADARG;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return CODETR_E_TOO_LARGE;
  if (!aligned16(x_dev, w_dev, y_dev)) return CODETR_E_BADARG;
  if (hm_head_dim != 0 || hm_rows != 0) {
    if (hm_head_dim <= 0 || hm_rows <= 0 || hm_head_dim % 8 != 0 || N % hm_head_dim != 0 || M % hm_rows != 0) return CODETR_E_UNSUPPORTED;
  }
  if (!xs_applicable(M, N, K, hm_head_dim) || K == 64) return CODETR_E_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch_ks(K, [&](auto ks) {
    return launch_xs_res<BFloatT, ks(), 0, HalfT>(st, x_dev, w_dev, bias_dev, nullptr, y_dev, row_mask_dev, (int)M, (int)N,
                                                  (int)hm_rows, hm_head_dim);
  });
}

}  // extern "C"
