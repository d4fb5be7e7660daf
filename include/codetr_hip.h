/*
 * codetr_hip.h -- C ABI of libcodetr_hip.so, the MI355X (gfx950) native library that
 * replaces the reference's codetr/csrc for the Co-DETR inference hot path.
 *
 * Boundary rules (same for every entry point):
 *   - extern "C", plain pointers and sizes; no torch / ATen types cross this line.
 *   - every pointer named *_dev is DEVICE memory owned by the caller (in practice the
 *     PyTorch-ROCm caching allocator); it is borrowed for the duration of the
 *     asynchronous launch and must stay alive until the stream reaches that point.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *     Work is enqueued and the call returns; nothing here synchronises, allocates,
 *     or reads device data on the host, so every entry point is hipGraph-capturable.
 *   - return value: 0 on success; a positive hipError_t value if the launch failed;
 *     a negative CODETR_E_* value if the arguments break the reference's contract
 *     (the reference raises c10::Error via AT_ASSERTM for those; the Python host
 *     turns every non-zero code into a RuntimeError -- nothing fails silently).
 *   - stateless and re-entrant.
 *
 * Which reference interface each entry point replaces is cited per function
 * (paths relative to the reference tree).
 */
#ifndef CODETR_HIP_H_
#define CODETR_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_E_BADARG (-1)      /* null pointer / non-positive dimension                       */
#define CODETR_E_IM2COL_STEP (-2) /* batch % min(batch, im2col_step) != 0  (ms_deform_attn.cu:924-926) */
#define CODETR_E_TOO_LARGE (-3)   /* a per-image extent exceeds the kernel's 32-bit in-image offsets  */
#define CODETR_E_UNSUPPORTED (-4) /* shape outside what the kernel family implements             */

/* ABI version of this header; bumped on any signature change. */
#define CODETR_HIP_ABI_VERSION 54
int codetr_hip_abi_version(void);
/* Human-readable message for a code returned by any entry point (static storage). */
const char *codetr_hip_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * Multi-scale deformable attention, forward.
 *
 * Replaces:  ms_deformable_im2col_cuda<T>(stream, value, spatial_shapes, level_start_index,
 *            sampling_loc, attn_weight, batch, spatial_size, num_heads, channels, num_levels,
 *            num_query, num_point, out)              codetr/csrc/ms_deform_attn.cu:762-779
 *            and the argument contract of
 *            codetr::ms_deform_attn_forward_reference codetr/csrc/ms_deform_attn.cu:899-956
 *            (also what the TensorRT plugin's enqueue hands over,
 *             codetr/csrc/deformable_attention_plugin.cpp:285-355).
 *
 *   value_dev          [B, S, M, D]          T     flattened multi-level value map
 *   spatial_shapes_dev [L, 2]                int64 (H_l, W_l), read ON DEVICE (cu:236-239)
 *   level_start_dev    [L]                   int64 first row of level l inside S
 *   loc_dev            [B, Nq, M, L, P, 2]   T     (x, y) normalised to [0, 1]
 *   weight_dev         [B, Nq, M, L, P]      T
 *   out_dev            [B, Nq, M*D]          T     every element is written (no pre-zeroing
 *                                                  needed; the reference zero-fills then
 *                                                  overwrites, cu:936)
 *   im2col_step        kept for API parity: validated exactly like cu:924-926, then the whole
 *                      batch is processed by one launch.
 *
 * Semantics: out[b,q,m,c] = sum_l sum_p w[b,q,m,l,p] * bilinear(value_l[b,:,m,c], x*W_l-0.5,
 * y*H_l-0.5) with zero padding per corner and the (-1, size) range gate (cu:31-77, 246-252).
 * Coordinates, bilinear weights and the accumulation are fp32 for f16/bf16/f32 tensors
 * (fp64 for f64) with one rounding at the store.
 * ------------------------------------------------------------------------------------------ */
int codetr_msda_forward_f16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                            const int64_t *level_start_dev, const void *loc_dev, const void *weight_dev,
                            int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P, int64_t im2col_step,
                            void *out_dev);
int codetr_msda_forward_bf16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                             const int64_t *level_start_dev, const void *loc_dev, const void *weight_dev,
                             int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P, int64_t im2col_step,
                             void *out_dev);
int codetr_msda_forward_f32(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                            const int64_t *level_start_dev, const void *loc_dev, const void *weight_dev,
                            int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P, int64_t im2col_step,
                            void *out_dev);
int codetr_msda_forward_f64(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                            const int64_t *level_start_dev, const void *loc_dev, const void *weight_dev,
                            int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P, int64_t im2col_step,
                            void *out_dev);

/* The windowed kernel behind codetr_msda_forward_f16 / _bf16 for encoder-shaped calls (round 6, csrc/msda_op4.hip; the
 * same op, reference codetr/csrc/ms_deform_attn.cu:211-261, 762-779): Nq == S, 5 levels x 4 points, 32-channel heads, fp16
 * or bf16.  Per (16 x 16 region of the finest level, head) the value rows the region's samples can reach are staged in LDS
 * with a zero border, sampling locations / attention weights reach the lanes through LDS records, samples outside a window
 * take a fix-up path with the reference's gate -- results as the general kernel's for ANY locations (fp32 blend, one
 * rounding to nearest even at the store; bf16 is widened exactly).  codetr_msda_forward_f16 / _bf16 call it by themselves;
 * the entry points are exported for tests and benchmarks:
 *   codetr_msda_op4_supported    the host-visible part of the routing test (types, counts, 32-bit offset ranges); the
 *                                pyramid itself is a device tensor and is judged on the device (csrc/msda_op4_plan.h).
 *                                elem_bytes 2 stands for both 16-bit types
 *   codetr_msda_op4_forward_f16  launches the windowed kernel only: where the device-side plan does not apply its workgroups
 *   codetr_msda_op4_forward_bf16 return without writing `out` (codetr_msda_forward_f16 / _bf16 launch the general kernel
 *                                behind it, which evaluates the same plan and returns at once where this kernel did the
 *                                work) */
int codetr_msda_op4_supported(int elem_bytes, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P);
int codetr_msda_op4_forward_f16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                                const int64_t *level_start_dev, const void *loc_dev, const void *weight_dev, int64_t B,
                                int64_t S, int M, int D, int L, int64_t Nq, int P, void *out_dev);
int codetr_msda_op4_forward_bf16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                                 const int64_t *level_start_dev, const void *loc_dev, const void *weight_dev, int64_t B,
                                 int64_t S, int M, int D, int L, int64_t Nq, int P, void *out_dev);

/* ------------------------------------------------------------------------------------------
 * Multi-scale deformable attention with its prologue fused.
 *
 * Same gather as above, but the kernel also performs the steps the reference's module runs between
 * its two projections and the op (codetr/multi_scale_deformable_attention.py:180-196): softmax over
 * the L*P attention logits of each (query, head), and sampling_locations = reference point +
 * normalised offset.  The sampling-location and attention-weight tensors (131 MB + 65 MB per encoder
 * call at 1920x1280 fp16) never exist.  The unfused entry points above remain the op's public form.
 *
 *   offsets_dev [B*Nq rows, offsets_row_stride]  columns [0, M*L*P*2): (x, y) offsets, order (m, l, p, xy)
 *   logits_dev  [B*Nq rows, logits_row_stride]   columns [0, M*L*P): raw attention logits, order (m, l, p)
 *               (both may be column ranges of ONE fused projection output: pass the same row stride
 *                and pointers offset by the column start)
 *   ref_dev     [B, Nq, L, ref_dim]  ref_dim 2: (x, y), loc = ref + off / (W_l, H_l)
 *                                    ref_dim 4: (x, y, w, h), loc = ref_xy + off / P * ref_wh * 0.5
 *   value_head_major  0: value_dev is [B, S, M, D] (the op's layout);
 *                     1: value_dev is [B, M, S, D] (written that way by codetr_linear_*'s head-major
 *                        epilogue): the x0/x1 neighbours of a sample are one 128-byte line, a pair is
 *                        served by twice the lanes and half the loads (D*2 bytes in {64, 128})
 * fp32 softmax / locations; 16-bit storage only; D*2 bytes per head must be 32, 64 or 128.
 * ------------------------------------------------------------------------------------------ */
int codetr_msda_fused_forward_f16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                                  const int64_t *level_start_dev, const void *offsets_dev, int64_t offsets_row_stride,
                                  const void *logits_dev, int64_t logits_row_stride, const void *ref_dev, int ref_dim,
                                  int value_head_major, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P,
                                  void *out_dev);
int codetr_msda_fused_forward_bf16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                                   const int64_t *level_start_dev, const void *offsets_dev, int64_t offsets_row_stride,
                                   const void *logits_dev, int64_t logits_row_stride, const void *ref_dev, int ref_dim,
                                   int value_head_major, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P,
                                   void *out_dev);
/* The same with ref_dev in fp32 ([B, Nq, L, ref_dim] float, 8-byte aligned) while value / offsets / logits / output keep
 * their 16-bit type: a 16-bit model's reference points (sigmoid outputs in [0, 1]) resolve a coordinate to 1/2048,
 * a quarter pixel on a 480-wide level; codetr_query_sine_embed_f16 writes them unrounded for the decoder's layers. */
int codetr_msda_fused_forward_ref32_f16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                                        const int64_t *level_start_dev, const void *offsets_dev,
                                        int64_t offsets_row_stride, const void *logits_dev, int64_t logits_row_stride,
                                        const void *ref_dev, int ref_dim, int value_head_major, int64_t B, int64_t S,
                                        int M, int D, int L, int64_t Nq, int P, void *out_dev);
int codetr_msda_fused_forward_ref32_bf16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                                         const int64_t *level_start_dev, const void *offsets_dev,
                                         int64_t offsets_row_stride, const void *logits_dev, int64_t logits_row_stride,
                                         const void *ref_dev, int ref_dim, int value_head_major, int64_t B, int64_t S,
                                         int M, int D, int L, int64_t Nq, int P, void *out_dev);

/* ------------------------------------------------------------------------------------------
 * Encoder self-attention form of the fused op (LDS-staged gather), for DetrTransformerEncoder
 * (codetr/transformer.py:81-92), where the queries ARE the pixels of the flattened multi-level map (Nq == S, query q =
 * pixel q) and reference_points are 2-d (get_reference_points, codetr/transformer.py:280-305).
 * (The round-3/4 forms codetr_msda_encoder_forward[_win]_* left the library in round 6 with their kernels:
 * tools/micro/experiments/msda_encoder_v3.hip.)
 * ------------------------------------------------------------------------------------------ */
/* Round-5 form of the encoder kernel ("v4", csrc/msda_encoder4.hip): the same op -- ms_deform_attn.cu:31-77, 211-261 with
 * the softmax / sampling-location prologue of multi_scale_deformable_attention.py:180-196 and the reference points of
 * transformer.py:280-305 -- for fp16, L == 5, P == 4, D == 32, with the (offsets | logits) projection handed over in a
 * LANE-MAJOR PACKED layout so that a quad lane of the gather fetches all it needs with two 16-byte loads:
 *   packed_dev        [B * S][packed_row_stride] fp16, packed_row_stride >= 64 M and a multiple of 8; for head m and
 *                     point p (= the quad lane), the 16 halves at columns 64 m + 16 p .. + 15 are
 *                       (x, y) offset of (m, level 0, p), ... , (m, level 4, p)        10 halves   [sampling_offsets rows
 *                       logit of (m, level 0, p), ... , (m, level 4, p)                 5 halves    ((m L + l) P + p) 2 + xy,
 *                       one pad half (ignored)                                                       attention_weights rows (m L + l) P + p]
 *                     i.e. the output of the (sampling_offsets | attention_weights) Linear with its weight rows permuted
 *                     once on the host (codetr_msda_pack_projection_index gives the permutation).
 *   valid_counts_dev  [B][L][2] fp32, required: the reference points are computed in fp32 from the query's pixel centre
 *                     and the valid pixel counts (see codetr_msda_encoder_forward_win_f16).
 *   windows_host      [M][L][4] int8 as above.  A window may exceed the level: it is clamped to the image plus a one-pixel
 *                     ZERO border (corners outside the image read zeros from LDS, ms_deform_attn.cu:52-71), so a wide
 *                     window on a coarse level keeps the whole level resident.
 *   region_w/region_h region of a workgroup in pixels of the finest level; threads: 256 | 512 per workgroup.  A region may
 *                     hold at most 3 * threads / 4 queries (CODETR_E_UNSUPPORTED otherwise).
 *   value_head_major  0: value_dev is the op's [B, S, M, D]; 1: [B, M, S, D] (each head's map contiguous, what
 *                     codetr_linear_* writes with hm_head_dim = D): a staged window row is then one contiguous run.
 * Samples outside the windows are added from global memory with the reference's gate / corner logic: windows change
 * speed, never results beyond the rounding of the packed blend (same tolerance statement as the _win entry).
 * codetr_msda_encoder_packed_lds_bytes: LDS bytes per workgroup such a launch needs, or a negative CODETR_E_* code.
 * codetr_msda_pack_projection_index: idx[64 M] (host): source row of the concatenated [M L P 2 + M L P] projection for
 * every packed output column, -1 for the pad columns. */
int codetr_msda_encoder_forward_packed_f16(void *stream, const void *value_dev, const int64_t *level_shapes_host,
                                           const void *packed_dev, int64_t packed_row_stride,
                                           const float *valid_counts_dev, int64_t B, int64_t S, int M, int D, int L, int P,
                                           const int8_t *windows_host, int region_w, int region_h, int threads,
                                           int value_head_major, void *out_dev);
/* The same for a bf16 model: packed projection and output are bf16, the VALUE MAP IS FP16 (value_f16_dev; written by
 * codetr_linear_bf16_f16out): the blend runs on packed halves either way -- gfx950 has no packed bf16 FMA -- and an fp16
 * value map keeps three more mantissa bits of the projection's fp32 accumulators than a bf16 one would.  Offsets and logits
 * are widened exactly; the result is rounded to bf16 once. */
int codetr_msda_encoder_forward_packed_bf16(void *stream, const void *value_f16_dev, const int64_t *level_shapes_host,
                                            const void *packed_dev, int64_t packed_row_stride,
                                            const float *valid_counts_dev, int64_t B, int64_t S, int M, int D, int L, int P,
                                            const int8_t *windows_host, int region_w, int region_h, int threads,
                                            int value_head_major, void *out_dev);
int64_t codetr_msda_encoder_packed_lds_bytes(const int64_t *level_shapes_host, int M, int L, int P,
                                             const int8_t *windows_host, int region_w, int region_h, int threads);
int codetr_msda_pack_projection_index(int M, int L, int P, int32_t *idx_host);

/* ------------------------------------------------------------------------------------------
 * Patch gather of the Swin stem (mmdet PatchEmbed: Conv2d(C, E, k, stride k) with "corner" zero padding, reference
 * codetr/swin.py:13, 567; equivalent source codetr/transformer_mmcv.py:100-210).  The convolution over
 * non-overlapping patches is a GEMM: this call writes its left operand,
 *   out[(b, ty, tx)][(c, ky, kx)] = x[b, c, k ty + ky, k tx + kx]   (0 beyond the image and for columns >= C k k),
 * in the column order of conv.weight.view(E, C k k), so that codetr_linear_* with the weight padded to kpad columns
 * produces the token-major [B, ceil(H/k) ceil(W/k), E] map directly (no NCHW round trip, no flatten / transpose).
 *   x_dev   [B, C, H, W]  16-bit elements (fp16 or bf16: pure data movement), 8-byte aligned
 *   out_dev [B * ceil(H/k) * ceil(W/k), kpad]  same element type, 16-byte aligned
 * Implemented for k == 4, kpad == 64 (C <= 4): CODETR_E_UNSUPPORTED otherwise.
 * ------------------------------------------------------------------------------------------ */
int codetr_patch_im2col_b16(void *stream, const void *x_dev, int64_t B, int C, int64_t H, int64_t W, int k, int kpad,
                            void *out_dev);

/* k x k / stride / zero-padding patches of a token-major map, for convolutions run as GEMMs on token-major data
 * (the neck's extra level: Conv2d(1536, 256, 3, stride 2, padding 1) of mmdet's ChannelMapper, built at
 * codetr/codetr.py:53-54 from configs lsj:40-47):
 *   out[(b, oy, ox)][(ky, kx, c)] = x[b, oy*stride + ky - pad, ox*stride + kx - pad, c]   (0 outside the map)
 *   x_dev [B, H, W, C] 16-bit elements, C % 8 == 0;  out_dev [B*Ho*Wo, k*k*C], Ho = (H + 2 pad - k) / stride + 1.
 * The GEMM weight is conv.weight permuted to [C_out, (ky, kx, c)]. */
int codetr_im2col_tokens_b16(void *stream, const void *x_dev, int64_t B, int64_t H, int64_t W, int64_t C, int k,
                             int stride, int pad, void *out_dev);

/* ------------------------------------------------------------------------------------------
 * Native ResNet-50 backbone (16-bit, token-major).  Replaces mmdet's ResNet (depth 50, style 'pytorch', frozen BN)
 * that the R50 config builds, configs/co_dino_5scale_r50_lsj_8xb2_1x_coco.py:22-31: every Conv2d + frozen BatchNorm
 * (+ ReLU) (+ residual add + ReLU) and the stem's max pool.  The host folds each BN into its conv (weight w gamma /
 * sqrt(var + eps), bias beta - mean gamma / sqrt(var + eps), in fp32, rounded once to T).
 *
 * Convolution on a token-major map as an implicit GEMM (no im2col buffer):
 *   y[b, oy, ox, n] = act(sum_{ky, kx, c} x[b, oy s + ky - pad, ox s + kx - pad, c] w[n, (ky, kx, c)] + bias[n])
 *                     (+ residual[b, oy, ox, n]), zero outside the map; act and residual exactly as codetr_linear_*
 *                     (act 3 = ReLU after the residual)
 *   x_dev        [B, H, W, C]      T (f16 / bf16), C % 64 == 0
 *   w_dev        [Cout, k k C]     T, columns ordered (ky, kx, c): conv.weight.permute(0, 2, 3, 1)
 *   bias_dev     [Cout] or NULL;   residual_dev [B, Ho, Wo, Cout] or NULL;   y_dev [B, Ho, Wo, Cout], Cout % 8 == 0
 *   Ho = (H + 2 pad - k) / stride + 1 (likewise Wo).  k in {1, 3}, stride in {1, 2}, 0 <= pad < k, act 0..3:
 *   CODETR_E_UNSUPPORTED otherwise.  Every pointer 16-byte aligned.  fp32 accumulation on the MFMA units, one rounding
 *   at the store (the residual is added to the rounded result, as in codetr_linear_*).
 * Serves the bottlenecks' 3x3 convs (stride 1 and 2) and the stride-2 1x1 downsample convs; the stride-1 1x1 convs
 * are plain GEMMs over tokens (codetr_linear_*).
 * ------------------------------------------------------------------------------------------ */
int codetr_conv_tokens_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                           const void *residual_dev, void *y_dev, int64_t B, int64_t H, int64_t W, int64_t C,
                           int64_t Cout, int k, int stride, int pad, int act);
int codetr_conv_tokens_bf16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                            const void *residual_dev, void *y_dev, int64_t B, int64_t H, int64_t W, int64_t C,
                            int64_t Cout, int k, int stride, int pad, int act);

/* Gather of the stem's overlapping-window convolution (Conv2d(3, 64, 7, stride 2, padding 3) on the NCHW image):
 *   out[(b, oy, ox)][(c, ky, kx)] = x[b, c, oy s + ky - pad, ox s + kx - pad]   (0 outside the image and for columns
 *   >= C k k), the column order of conv.weight.view(Cout, C k k); codetr_linear_* with the weight padded to kpad columns
 *   then computes the convolution (the overlapping-window form of codetr_patch_im2col_b16).
 *   x_dev [B, C, H, W] 16-bit;  out_dev [B Ho Wo, kpad] same type, 16-byte aligned;  kpad % 8 == 0 and kpad >= C k k
 *   (CODETR_E_UNSUPPORTED otherwise). */
int codetr_conv_im2col_nchw_b16(void *stream, const void *x_dev, int64_t B, int C, int64_t H, int64_t W, int k,
                                int stride, int pad, int kpad, void *out_dev);

/* Max pool on a token-major map, F.max_pool2d(x, 3, 2, 1) semantics: padding never wins, a NaN in the window is
 * returned (torch's rule: the last NaN of the row-major scan), the result is exact (the winner's bits are stored).
 *   x_dev [B, H, W, C] 16-bit, C % 8 == 0;  y_dev [B, Ho, Wo, C], Ho = (H - 1) / 2 + 1;  is_bf16: 0 = fp16, 1 = bf16.
 *   k == 3, stride == 2, pad == 1 only (CODETR_E_UNSUPPORTED otherwise); 16-byte aligned bases. */
int codetr_maxpool_tokens_b16(void *stream, const void *x_dev, int64_t B, int64_t H, int64_t W, int64_t C, int k,
                              int stride, int pad, int is_bf16, void *y_dev);

/* Row-wise top-k of 16-bit floats: the two selections of the detection head -- the two-stage proposals
 * (torch.topk(enc_outputs_class.max(-1)[0], 900, dim=1), reference codetr/transformer.py:560-561) and the final
 * detections (cls_score.view(B, -1).topk(300), reference codetr/co_dino_head.py:183-186).
 *   x_dev       [rows, n]  f16 / bf16, contiguous
 *   values_dev  [rows, k]  same type, or NULL;   indices_dev [rows, k] int64
 * Sorted: descending value, ties by ascending index, NaN first (torch's NaN rule; torch leaves the tie order open).
 * k <= 1024, k <= n < 2^24: CODETR_E_UNSUPPORTED otherwise. */
int codetr_topk_f16(void *stream, const void *x_dev, int64_t rows, int64_t n, int k, void *values_dev,
                    int64_t *indices_dev);
int codetr_topk_bf16(void *stream, const void *x_dev, int64_t rows, int64_t n, int k, void *values_dev,
                     int64_t *indices_dev);

/* The same selection with a long row cut over several workgroups (the 204 600-element proposal row of one image):
 *   codetr_topk_chunks         how many equal pieces to cut a row into (1: call codetr_topk_*) and the workspace needed
 *   codetr_topk_chunked_*      pass 1: top k of every piece (rows * chunks workgroups); pass 2: top k of the
 *                              chunks * k candidates, mapped back to row indices.  Same result, same stable order.
 * Caller-owned workspace (16-byte aligned), no allocation, hipGraph-capturable. */
int64_t codetr_topk_chunks(int64_t n, int k, int64_t rows, int64_t *workspace_bytes);
int codetr_topk_chunked_f16(void *stream, const void *x_dev, int64_t rows, int64_t n, int k, int chunks,
                            void *values_dev, int64_t *indices_dev, void *workspace_dev, int64_t workspace_bytes);
int codetr_topk_chunked_bf16(void *stream, const void *x_dev, int64_t rows, int64_t n, int k, int chunks,
                             void *values_dev, int64_t *indices_dev, void *workspace_dev, int64_t workspace_bytes);

/* Name of the kernel variant the arguments above would dispatch to ("tiled_d32x8", "scalar", ...).
 * Pure host function; lets tests assert that the model shape takes the tiled path. */
const char *codetr_msda_variant(int elem_bytes, int M, int D, int L, int P);

/* ------------------------------------------------------------------------------------------
 * Fused linear layer:  y[M,N] = act(x[M,K] . w[N,K]^T + bias[N]) (+ residual[M,N])
 *
 * Replaces, for the nn.Linear layers of the hot path, the ATen call sequence the reference runs
 * per layer (addmm / bias add / ReLU or GELU / residual add as separate kernels):
 *   Swin qkv / proj / MLP           codetr/swin.py:91-115, codetr/transformer_mmcv.py:484-500
 *   MSDA value / offsets / weights / output projections
 *                                   codetr/multi_scale_deformable_attention.py:173-213
 *   encoder / decoder FFN, MHA projections, reference-point MLP, class / box branches
 *                                   codetr/transformer.py:218, 551-557; codetr/co_dino_head.py:169-177
 *
 *   x_dev        [M, K]  row-major, dense            T (f16 / bf16)
 *   w_dev        [N, K]  row-major (nn.Linear.weight) T
 *   bias_dev     [N] or NULL                          T
 *   residual_dev [M, N] or NULL (added AFTER the activation, as `identity + ffn(x)` does)   T
 *   row_mask_dev [M] uint8/bool or NULL: rows with mask value 1 (any non-zero value but 2) are written as
 *                zeros (before the residual) -- `value.masked_fill(key_padding_mask[..., None], 0.0)` of
 *                codetr/multi_scale_deformable_attention.py:174-175 folded into value_proj.  Mask value 2: the
 *                INPUT row counts as zeros, y = act(bias) -- `memory * keep` of apply_mask_to_proposal_and_memory
 *                (codetr/transformer.py:365-380) folded into enc_output
 *   y_dev        [M, N]  (may alias residual_dev)     T
 *   act          0 = none, 1 = ReLU, 2 = GELU (erf form, nn.GELU default), 3 = ReLU applied AFTER the residual:
 *                y = relu(x . w^T + bias + residual), rounded as act 0 + residual and then clamped (the ResNet
 *                bottleneck's relu(bn3(conv3(x)) + identity)); with no residual act 3 is act 1.  Act 3 exists on
 *                codetr_linear_f16 / _bf16 and codetr_conv_tokens_* only: every other linear entry rejects it
 *   hm_rows, hm_head_dim   0, 0: y is row-major [M, N].  Otherwise the rows are (batch, position) with
 *                hm_rows positions per batch and the columns (head, channel) with hm_head_dim channels per
 *                head, and y is written HEAD-MAJOR: y[b][head][position][channel] -- the value-map layout
 *                of codetr_msda_fused_forward_*(value_head_major = 1).  Needs N % 8 == 0, no residual.
 *
 * fp32 accumulation on the MFMA units, one rounding at the store.  K must be a multiple of 64
 * (every Linear of the model is; CODETR_E_UNSUPPORTED otherwise); x / w 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int codetr_linear_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                      const void *residual_dev, const void *row_mask_dev, void *y_dev, int64_t M, int64_t N,
                      int64_t K, int act, int64_t hm_rows, int hm_head_dim);
int codetr_linear_bf16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                       const void *residual_dev, const void *row_mask_dev, void *y_dev, int64_t M, int64_t N,
                       int64_t K, int act, int64_t hm_rows, int hm_head_dim);
/* bf16 operands, FP16 output (no activation, no residual; row mask and head-major destination as above): the value
 * projection in front of codetr_msda_encoder_forward_packed_bf16, whose staged value map is fp16 whatever the model's
 * type (its blend runs on packed halves; gfx950 has no packed bf16 FMA).  fp32 accumulators rounded once to fp16 -- three
 * more mantissa bits than the bf16 store they replace.  Large short-K problems only (the X-stationary kernel: K in
 * {192, 256}, M >= 32 768, 128 <= N <= 1536); CODETR_E_UNSUPPORTED otherwise. */
int codetr_linear_bf16_f16out(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                              const void *row_mask_dev, void *y_dev, int64_t M, int64_t N, int64_t K,
                              int64_t hm_rows, int hm_head_dim);
/* The encoder self-attention's two projections of one token row as ONE launch (reference
 * codetr/multi_scale_deformable_attention.py:161-162 `query = query + query_pos`, :173-176 value_proj + masked_fill,
 * :177-182 sampling_offsets | attention_weights; in the encoder `value` IS `query`):
 *     value  [M, N_value]  = x @ W[:N_value]^T + b[:N_value]            rows with row_mask != 0 zeroed; head-major
 *                            destination [M / hm_rows][N_value / hm_head_dim][hm_rows][hm_head_dim] if hm_head_dim != 0
 *     packed [M, N_packed] = (x + pos) @ W[N_value:]^T + b[N_value:]    x + pos rounded to the operand type first, exactly
 *                            as the separate add; row-major
 * w_dev [N_value + N_packed, K] and bias_dev are the two layers' parameters concatenated (value rows first).  x and pos
 * are each read once for both products -- as two launches x is read twice (419 MB of 2.5 GB at four 1920x1280 images)
 * and the value projection pays its own prologue.  _bf16: operands, packed output bf16; the value map is FP16 (see
 * codetr_linear_bf16_f16out).  X-stationary kernel: K == 256, N_value % 64 == 0, N_packed % 8 == 0, N_value + N_packed
 * <= 1536, M >= 32 768, 16-byte aligned pointers; CODETR_E_UNSUPPORTED otherwise (the caller then launches the two GEMMs). */
int codetr_encoder_projections_f16(void *stream, const void *x_dev, const void *pos_dev, const void *w_dev,
                                   const void *bias_dev, const void *row_mask_dev, void *value_dev, void *packed_dev,
                                   int64_t M, int64_t N_value, int64_t N_packed, int64_t K, int64_t hm_rows,
                                   int hm_head_dim);
int codetr_encoder_projections_bf16(void *stream, const void *x_dev, const void *pos_dev, const void *w_dev,
                                    const void *bias_dev, const void *row_mask_dev, void *value_f16_dev,
                                    void *packed_dev, int64_t M, int64_t N_value, int64_t N_packed, int64_t K,
                                    int64_t hm_rows, int hm_head_dim);
/* Round 6: the same launch with the positional operand GENERATED in the kernel instead of read.  `pos` of the encoder is the
 * sine positional encoding + level embedding (reference positional_encoding.py:58-93, transformer.py:508-519: what
 * codetr_sine_pos_tokens_* writes): a function of the token's (level, y, x) and of the running sums of the padding mask.  The
 * kernel re-derives a row's two normalised coordinates from the running sums (8 bytes per token instead of the row's 512) and
 * evaluates its channels with the same fp32 operations in the same order as codetr_sine_pos_tokens_*, so value / packed are
 * BIT-IDENTICAL to codetr_encoder_projections_* fed the tensor that entry writes (tests/test_encoder_projections_gpu.py).
 *   ycum0..4 / xcum0..4   per level (nullptr beyond num_levels): running sums of the not-mask along y / x, [B, H_l, W_l] fp32
 *                         (the inputs of codetr_sine_pos_tokens_*);  level_shapes_host [num_levels][2] = (H_l, W_l), sum = S
 *   level_embed_dev       [num_levels, K] in the operands' type, or nullptr;  temperature .. normalize as codetr_sine_pos_tokens_*
 *   M = B * S rows;  the other arguments as codetr_encoder_projections_*. */
int codetr_encoder_projections_posgen_f16(void *stream, const void *x_dev, const float *ycum0, const float *ycum1,
                                          const float *ycum2, const float *ycum3, const float *ycum4, const float *xcum0,
                                          const float *xcum1, const float *xcum2, const float *xcum3, const float *xcum4,
                                          const int64_t *level_shapes_host, int num_levels, const void *level_embed_dev,
                                          float temperature, float scale, float eps, float offset, int normalize,
                                          const void *w_dev, const void *bias_dev, const void *row_mask_dev, void *value_dev,
                                          void *packed_dev, int64_t M, int64_t S, int64_t N_value, int64_t N_packed, int64_t K,
                                          int64_t hm_rows, int hm_head_dim);
int codetr_encoder_projections_posgen_bf16(void *stream, const void *x_dev, const float *ycum0, const float *ycum1,
                                           const float *ycum2, const float *ycum3, const float *ycum4, const float *xcum0,
                                           const float *xcum1, const float *xcum2, const float *xcum3, const float *xcum4,
                                           const int64_t *level_shapes_host, int num_levels, const void *level_embed_dev,
                                           float temperature, float scale, float eps, float offset, int normalize,
                                           const void *w_dev, const void *bias_dev, const void *row_mask_dev,
                                           void *value_f16_dev, void *packed_dev, int64_t M, int64_t S, int64_t N_value,
                                           int64_t N_packed, int64_t K, int64_t hm_rows, int hm_head_dim);

/* Which of the three kernels behind codetr_linear_* serves a (16-byte aligned) problem: "tile128" (128x128 tiles, the
 * general kernel), "tile256" (256x256 tiles, one workgroup per CU), "xs" (X-stationary short-K kernel) or
 * "unsupported" (K % 64 != 0).  Pure function of the arguments (the library reads no environment variable); it is the
 * same routine the launcher consults, so tests can assert which kernel a model shape exercises. */
const char *codetr_linear_variant(int64_t M, int64_t N, int64_t K, int act, int has_residual, int hm_head_dim);

/* y = (x + x_add) . w^T + bias with the element-wise add folded into the operand load of the short-K kernel:
 * `query + query_pos` in front of the (offsets | logits) projection of MultiScaleDeformableAttention
 * (codetr/multi_scale_deformable_attention.py:161-162, 177-179) without a separate add kernel or a stored sum.
 * x + x_add is rounded to T first, exactly as the stand-alone fp16 / bf16 add.  x_add_dev [M, K] like x_dev.
 * Only where the X-stationary kernel applies (K in {192, 256}, 128 <= N <= 1536, N % 8 == 0, M >= 32768):
 * CODETR_E_UNSUPPORTED otherwise -- callers then add and call codetr_linear_*. */
int codetr_linear_xadd_f16(void *stream, const void *x_dev, const void *x_add_dev, const void *w_dev,
                           const void *bias_dev, void *y_dev, int64_t M, int64_t N, int64_t K);
int codetr_linear_xadd_bf16(void *stream, const void *x_dev, const void *x_add_dev, const void *w_dev,
                            const void *bias_dev, void *y_dev, int64_t M, int64_t N, int64_t K);

/* y = act(LayerNorm(x) . w^T + bias) with the LayerNorm applied to the rows as they are loaded by the short-K kernel
 * (the whole row is that kernel's stationary operand): Swin's pre-norm blocks, norm1 -> qkv and norm2 -> fc1 (reference
 * codetr/swin.py:345-386), where nothing else reads the normalised tensor.  fp32 two-pass statistics, the normalised
 * row rounded to T before the product (what the separate kernel writes).  gamma / beta [K].
 * Only where the X-stationary kernel applies (K in {192, 256}, 128 <= N <= 1536, N % 8 == 0, M >= 32768):
 * CODETR_E_UNSUPPORTED otherwise -- callers then run codetr_layernorm_* and codetr_linear_*. */
int codetr_linear_ln_f16(void *stream, const void *x_dev, const void *ln_gamma_dev, const void *ln_beta_dev,
                         float ln_eps, const void *w_dev, const void *bias_dev, void *y_dev, int64_t M, int64_t N,
                         int64_t K, int act);
int codetr_linear_ln_bf16(void *stream, const void *x_dev, const void *ln_gamma_dev, const void *ln_beta_dev,
                          float ln_eps, const void *w_dev, const void *bias_dev, void *y_dev, int64_t M, int64_t N,
                          int64_t K, int act);

/* ------------------------------------------------------------------------------------------
 * FP8 (OCP e4m3) linear layer and its activation producers -- BASELINE config 5 ("fp8 weights + activations").
 * No reference counterpart (the reference's dtypes stop at half: codetr/csrc/ms_deform_attn.cu:946,
 * export.py:39-44); the layers served are the nn.Linears of codetr/swin.py:91-115, 345-355.
 *
 *   codetr_linear_fp8      y = act((x8 . w8^T) * x_scale * w_scale[n] + bias[n]) (+ residual)
 *                          x8 [M, K] / w8 [N, K] e4m3 bytes, K contiguous; w_scale [N] fp32 (per output channel);
 *                          x_scale: the static per-tensor scale the producer divided by; bias [N] / residual [M, N]
 *                          fp16 or NULL; y [M, N] fp16, or e4m3 = sat(y / out_scale) when out_is_fp8 (then no
 *                          residual).  fp32 accumulation with v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales).
 *                          K % 128 == 0, N % 8 == 0, 16-byte aligned bases; act as codetr_linear_*.
 *   codetr_cast_fp8_f16    y8[i] = sat(x[i] / scale), n % 8 == 0 elements
 *   codetr_layernorm_fp8_f16  LayerNorm over the last dimension C (fp32 statistics, result rounded to fp16 as the
 *                          fp16 model would) then sat(. / scale) -> e4m3; C % 8 == 0, C <= 4096
 * Saturation: values are clamped to +-448 (the largest finite e4m3) before conversion.
 * ------------------------------------------------------------------------------------------ */
int codetr_linear_fp8(void *stream, const void *x8_dev, const void *w8_dev, const float *w_scale_dev, float x_scale,
                      const void *bias_f16_dev, const void *residual_f16_dev, void *y_dev, int out_is_fp8,
                      float out_scale, int64_t M, int64_t N, int64_t K, int act);
int codetr_cast_fp8_f16(void *stream, const void *x_f16_dev, void *y8_dev, int64_t n, float scale);
int codetr_layernorm_fp8_f16(void *stream, const void *x_f16_dev, const void *gamma_f16_dev, const void *beta_f16_dev,
                             void *y8_dev, int64_t rows, int64_t C, float eps, float scale);

/* ------------------------------------------------------------------------------------------
 * The same path with MX BLOCK SCALES on the activations (no calibration, no static scale): every 32 consecutive
 * K-elements of an activation row share one e8m0 exponent byte (2^(byte - 127)) chosen by the producer from the block's
 * own maximum, and v_mfma_scale_f32_16x16x128_f8f6f4 applies it in hardware -- a lane's scale byte covers exactly the 32
 * operand bytes that lane holds.  Weights keep one fp32 scale per output channel (unit block scales in the instruction).
 *
 * Scale tensors: codetr_mx_scale_bytes(M, K) bytes for an activation [M, K], byte of (row m, block kb = k / 32) at
 *   (((kb >> 2) * MB + (m >> 7)) * 64 + (kb & 3) * 16 + (m & 15)) * 8 + ((m >> 4) & 7),   MB = ceil(M / 128)
 * (the 8 bytes a lane of the GEMM needs per 128-wide k-tile are contiguous: csrc/mx_scale.h).
 *
 *   codetr_linear_fp8mx          y = act((x8 (*) x_scales) . w8^T * w_scale[n] + bias[n]) (+ residual); y fp16, or -- when
 *                                y_scales_dev is given (no residual, N % 128 == 0) -- e4m3 with block scales along N, laid
 *                                out for a consumer GEMM over the same M rows whose K is this N
 *   codetr_cast_fp8mx_f16        x [rows, C] fp16 -> e4m3 + scales (C % 128 == 0)
 *   codetr_layernorm_fp8mx_f16   LayerNorm (as codetr_layernorm_fp8_f16) -> e4m3 + scales (C % 128 == 0)
 *   codetr_window_attention_fp8mx_f16  codetr_window_attention_f16 with its output as e4m3 + scales: one block per
 *                                (token, head) -- head_dim == 32 is the MX block
 * ------------------------------------------------------------------------------------------ */
int64_t codetr_mx_scale_bytes(int64_t M, int64_t K);
int codetr_linear_fp8mx(void *stream, const void *x8_dev, const void *x_scales_dev, const void *w8_dev,
                        const float *w_scale_dev, const void *bias_f16_dev, const void *residual_f16_dev, void *y_dev,
                        void *y_scales_dev, int64_t M, int64_t N, int64_t K, int act);
int codetr_cast_fp8mx_f16(void *stream, const void *x_f16_dev, void *y8_dev, void *y_scales_dev, int64_t rows, int64_t C);
int codetr_layernorm_fp8mx_f16(void *stream, const void *x_f16_dev, const void *gamma_f16_dev, const void *beta_f16_dev,
                               void *y8_dev, void *y_scales_dev, int64_t rows, int64_t C, float eps);
int codetr_window_attention_fp8mx_f16(void *stream, const void *qkv_dev, const void *qkv_bias_dev,
                                      const void *rel_bias_dev, void *out8_dev, void *out_scales_dev, int64_t B, int64_t H,
                                      int64_t W, int num_heads, int head_dim, int window_size, int shift);

/* ------------------------------------------------------------------------------------------
 * Small fp16 element-wise / gather kernels of the decoder and the detection head (csrc/small_ops.hip): the last
 * ATen launches of the fp16 forward, bit-identical to the ATen formulation (one fp16 rounding per operation).
 *   codetr_add_f16           out[i] = a[i % a_period] + b[i]  (`query + query_pos`, reference transformer_mmcv.py:400-404;
 *                            a_period < n broadcasts `a`, e.g. query_embed.weight over the batch); n, a_period % 8 == 0
 *   codetr_sigmoid_f16       out = 1 / (1 + exp(-x))            (co_dino_head.py:181)
 *   codetr_gather_rows_b16   out[b,k,:] = src[b, idx[b,k], :]   (transformer.py:562-566; 16-bit rows, C % 4 == 0)
 *   codetr_decode_boxes_f16  q = idx / C, label = idx % C, sigmoid -> cxcywh -> xyxy -> x (W,H,W,H) -> clamp
 *                            (co_dino_head.py:177-209 + mmdet bbox_cxcywh_to_xyxy); coords_unact [B,Nq,4] = box branch
 *                            output + reference (before the sigmoid); boxes [B,K,4] fp16, labels [B,K] int64
 * Every entry point of this group, codetr_query_sine_embed_* and codetr_encoder_geometry_* / codetr_row_max_* below have a
 * _bf16 twin (same formulas with bfloat16 roundings and finfo(bf16).max): a bf16 model's forward is all C-ABI launches too.
 *   codetr_valid_ratios_f16  out[b,l,j] = fp16(counts[b,l,j]) / level_wh[l,j]   (transformer.py:384-400);
 *                            out32 (may be NULL): counts / level_wh in fp32, unrounded
 * ------------------------------------------------------------------------------------------ */
int codetr_add_f16(void *stream, const void *a_dev, const void *b_dev, void *out_dev, int64_t n, int64_t a_period);
int codetr_add_bf16(void *stream, const void *a_dev, const void *b_dev, void *out_dev, int64_t n, int64_t a_period);
int codetr_sigmoid_f16(void *stream, const void *x_dev, void *out_dev, int64_t n);
int codetr_sigmoid_bf16(void *stream, const void *x_dev, void *out_dev, int64_t n);
int codetr_gather_rows_b16(void *stream, const void *src_dev, const int64_t *idx_dev, void *out_dev, int64_t B, int64_t S,
                           int64_t K, int64_t C);
int codetr_decode_boxes_f16(void *stream, const void *coords_unact_dev, const int64_t *idx_dev, void *boxes_dev,
                            int64_t *labels_dev, int64_t B, int64_t Nq, int64_t K, int num_classes, float img_w,
                            float img_h);
int codetr_decode_boxes_bf16(void *stream, const void *coords_unact_dev, const int64_t *idx_dev, void *boxes_dev,
                            int64_t *labels_dev, int64_t B, int64_t Nq, int64_t K, int num_classes, float img_w,
                            float img_h);
int codetr_valid_ratios_f16(void *stream, const float *counts_dev, const void *level_wh_f16_dev, void *out_dev,
                            float *out32_dev, int64_t B, int L);
int codetr_valid_ratios_bf16(void *stream, const float *counts_dev, const void *level_wh_bf16_dev, void *out_dev,
                            float *out32_dev, int64_t B, int L);

/* Split-K form of the same layer for problems with few output tiles and a long K -- the neck's extra
 * 3x3 / stride-2 level (codetr/codetr.py neck, mmdet ChannelMapper extra_convs) run as a GEMM over unfolded
 * patches is [600, 13824] x [256, 13824]^T: 10 output tiles, one pass leaves 246 CUs idle.
 *   codetr_linear_splitk_plan  returns the number of K ranges the library would use for (M, N, K) -- 1 means
 *                              "call codetr_linear_*" -- and the fp32 workspace it needs (splits * M * N * 4 bytes).
 *   codetr_linear_splitk_*     pass 1 writes one fp32 partial tile per (output tile, K range) into the workspace,
 *                              pass 2 sums the ranges in fp32 and applies bias / activation / row mask / residual
 *                              with the same semantics as codetr_linear_*.  `splits` must come from the plan.
 * The workspace is caller-owned device memory (16-byte aligned) so that the calls stay allocation-free and
 * hipGraph-capturable. */
int codetr_linear_splitk_plan(int64_t M, int64_t N, int64_t K, int64_t *workspace_bytes);
int codetr_linear_splitk_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                             const void *residual_dev, const void *row_mask_dev, void *y_dev, int64_t M, int64_t N,
                             int64_t K, int act, int splits, void *workspace_dev, int64_t workspace_bytes);
int codetr_linear_splitk_bf16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                              const void *residual_dev, const void *row_mask_dev, void *y_dev, int64_t M, int64_t N,
                              int64_t K, int act, int splits, void *workspace_dev, int64_t workspace_bytes);

/* Persistent form of codetr_linear_* for the large layers (Swin stages 0-3 -- reference codetr/swin.py:92-112,
 * 331-352 -- where TensorRT picked its own GEMM tactic): one resident workgroup per CU walks whole 256 x 256 tiles with
 * its operand stream running across tile boundaries (csrc/gemm_sk.hip); same semantics as codetr_linear_* without row
 * mask / head-major output.
 *   codetr_linear_sk_supported        1 when (M, N, K) is inside the kernel's domain (K % 64 == 0, K >= 128, N % 8 == 0)
 *   codetr_linear_sk_preferred        1 when it measured faster than codetr_linear_* on this class of problem
 *                                     (profiles/r04_gemm_sk.txt): hosts call codetr_linear_sk_* then
 *   codetr_linear_sk_workspace_bytes  size of the caller-owned workspace (fp32 partial tiles + ticket counters of the
 *                                     stream-K split) on the current device; it must be ZERO-FILLED ONCE before its
 *                                     first use -- every launch returns the counters to zero -- and must not be shared
 *                                     by launches that can run concurrently (one per stream); without the 0x40 flag
 *                                     it is not touched and may be NULL / 0
 *   codetr_linear_sk_*                flags: 0 (default); 0x40 = stream-K split of the left-over tiles (correct, measured
 *                                     slower at this model's K); 0x20 = one workgroup per tile (A/B only) */
int64_t codetr_linear_sk_workspace_bytes(void);
int codetr_linear_sk_supported(int64_t M, int64_t N, int64_t K);
int codetr_linear_sk_preferred(int64_t M, int64_t N, int64_t K, int act, int has_residual);
int codetr_linear_sk_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                         const void *residual_dev, void *y_dev, int64_t M, int64_t N, int64_t K, int act,
                         void *workspace_dev, int64_t workspace_bytes, int flags);
int codetr_linear_sk_bf16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                          const void *residual_dev, void *y_dev, int64_t M, int64_t N, int64_t K, int act,
                          void *workspace_dev, int64_t workspace_bytes, int flags);

/* Fused Swin MLP (round 6, csrc/swin_mlp.hip): y = x + fc2(GELU(fc1(LayerNorm(x)))) in one launch -- the second half of a
 * SwinBlock (reference codetr/swin.py:331-352: x = x + ffn(norm2(x)), FFN = Linear(C, 4C) -> GELU (erf) -> Linear(4C, C)),
 * for the stages whose MLP is bound by the bytes of its hidden activation: C = 192 / 384 (Swin-L stages 0 / 1).  The hidden
 * activation and norm2's output never leave the CU.
 *   x_dev / y_dev        [M, C] row-major, 16-bit storage (y may not alias x: rows are read twice)
 *   ln_gamma / ln_beta   [C], ln_eps: norm2
 *   w1_dev [4C, C], b1_dev [4C];  w2_packed_dev [C, 4C] = codetr_ffn_pack_w2_f16(fc2.weight);  b2_dev [C]
 * CODETR_E_UNSUPPORTED for other C.  Numerics: LayerNorm and GELU in fp32, each rounded to the storage type once; fp32
 * accumulation; fc2's output rounded before the identity is added (the reference's two roundings). */
int codetr_swin_mlp_supported(int64_t M, int64_t C, int64_t hidden);
int codetr_swin_mlp_f16(void *stream, const void *x_dev, const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps,
                        const void *w1_dev, const void *b1_dev, const void *w2_packed_dev, const void *b2_dev, void *y_dev,
                        int64_t M, int64_t C);
int codetr_swin_mlp_bf16(void *stream, const void *x_dev, const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps,
                         const void *w1_dev, const void *b1_dev, const void *w2_packed_dev, const void *b2_dev, void *y_dev,
                         int64_t M, int64_t C);

/* Ping-pong form of codetr_linear_sk_* (round 6, csrc/gemm_pp.hip) for the same layers (reference codetr/swin.py:92-112,
 * 331-352): the same persistent 256 x 256 tiles, operand ring and epilogue, but the two waves of every SIMD take turns --
 * one multiplies (32 MFMAs, nothing else) while the other reads its fragments from LDS and issues its LDS-DMA pieces, a
 * workgroup barrier between the segments, the second group of four waves one barrier behind the first.  Same semantics
 * and domain as codetr_linear_sk_* (no workspace, no stream-K split).
 *   codetr_linear_pp_supported   1 when (M, N, K) is inside the kernel's domain (K % 64 == 0, K >= 128, N % 8 == 0)
 *   codetr_linear_pp_preferred   1 where it measured faster than codetr_linear_* and codetr_linear_sk_*
 *                                (profiles/r06_gemm_pp.txt): hosts call codetr_linear_pp_* then
 *   codetr_linear_pp_*           flags: 0 (reserved: the measured variants of the main loop are kept out of the library,
 *                                tools/micro/experiments/gemm_pp_variants.hip) */
int codetr_linear_pp_supported(int64_t M, int64_t N, int64_t K);
int codetr_linear_pp_preferred(int64_t M, int64_t N, int64_t K, int act, int has_residual);
int codetr_linear_pp_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                         const void *residual_dev, void *y_dev, int64_t M, int64_t N, int64_t K, int act, int flags);
int codetr_linear_pp_bf16(void *stream, const void *x_dev, const void *w_dev, const void *bias_dev,
                          const void *residual_dev, void *y_dev, int64_t M, int64_t N, int64_t K, int act, int flags);

/* ------------------------------------------------------------------------------------------
 * Padding-mask pyramid: everything the detection transformer derives from img_masks, one launch.
 *
 * Replaces, per level: F.interpolate(img_masks, size=feat.shape[-2:]).to(bool) (codetr/co_dino_head.py:155),
 * not_mask.cumsum(1) / cumsum(2) (codetr/positional_encoding.py:78-79), the two sums of get_valid_ratio
 * (codetr/transformer.py:384-399) and mask.flatten(1) + cat (codetr/transformer.py:513-520).
 *
 *   img_mask_dev        [B, H_img, W_img], non-zero = padding; mask_elem_bytes = 1 (bool / uint8), 2 (fp16 / bf16)
 *                       or 4 (fp32): the reference hands over a float mask (inferencer.py:354-358) and tests
 *                       `.to(bool)`; -0.0 counts as zero, NaN as non-zero
 *   level_shapes_host   HOST array of 2*num_levels int64: (H_l, W_l) per level (num_levels <= 8)
 *   mask_flat_dev       [B, S] uint8, S = sum H_l*W_l: level masks (nearest-neighbour resize, ATen's index rule),
 *                       levels concatenated -- the transformer's mask_flatten
 *   ycum_dev, xcum_dev  fp32, S*B elements each; level l occupies [B, H_l, W_l] starting at element B*start_l:
 *                       running count of valid pixels down the columns / along the rows (the inputs of
 *                       codetr_sine_pos_tokens_f16)
 *   valid_counts_dev    [B, num_levels, 2] fp32: valid pixels in the first row (w) and first column (h); the host
 *                       divides by (W_l, H_l) in the model dtype to get valid_ratios
 * ------------------------------------------------------------------------------------------ */
int codetr_mask_pyramid(void *stream, const void *img_mask_dev, int64_t B, int64_t H_img, int64_t W_img,
                        int num_levels, const int64_t *level_shapes_host, void *mask_flat_dev, float *ycum_dev,
                        float *xcum_dev, float *valid_counts_dev, int mask_elem_bytes);

/* ------------------------------------------------------------------------------------------
 * Decoder query positions: sigmoid + valid-ratio scaling of the reference boxes and their sine embedding.
 *
 * Replaces the head of each DinoTransformerDecoder layer iteration, codetr/transformer.py:208-217
 * (reference_points_input = reference_points[:, :, None].sigmoid() * cat([valid_ratios, valid_ratios], -1)[:, None];
 * query_sine_embed = gen_sineembed_for_position(reference_points_input[:, :, 0, :], embed_dims // 2)) and
 * gen_sineembed_for_position, codetr/transformer.py:157-190 -- 27 ATen launches per layer.
 *
 *   ref_dev           [B, Nq, ref_dim] f16, ref_dim 2 or 4: reference points, unactivated (apply_sigmoid = 1)
 *                     or already in [0, 1] (apply_sigmoid = 0)
 *   valid_ratios_dev  [B, num_levels, 2] f16 (w, h)
 *   ref_in_dev        out [B, Nq, num_levels, ref_dim] f16: the MSDA reference points of the layer
 *   embed_dev         out [B, Nq, ref_dim * pos_feat] f16: blocks ordered (y, x[, w, h]); within a block channel
 *                     2k = sin, 2k+1 = cos of  v * 2 pi / temperature^(2k / pos_feat),  v = ref_in[b, q, 0, coord]
 * fp32 trigonometry on the f16-rounded ref_in; pos_feat % 8 == 0.
 *   valid_ratios32_dev / ref_in32_dev  NULL, or fp32 valid ratios [B, num_levels, 2] and an fp32 output
 *                     [B, Nq, num_levels, ref_dim]: the same reference points with the sigmoid and the scaling kept in
 *                     fp32 (for codetr_msda_fused_forward_ref32_*); the embedding is then taken from these.
 * ------------------------------------------------------------------------------------------ */
int codetr_query_sine_embed_f16(void *stream, const void *ref_dev, const void *valid_ratios_dev,
                                const float *valid_ratios32_dev, int64_t B, int64_t Nq, int ref_dim, int num_levels,
                                int pos_feat, float temperature, int apply_sigmoid, void *ref_in_dev,
                                float *ref_in32_dev, void *embed_dev);
int codetr_query_sine_embed_bf16(void *stream, const void *ref_dev, const void *valid_ratios_dev,
                                const float *valid_ratios32_dev, int64_t B, int64_t Nq, int ref_dim, int num_levels,
                                int pos_feat, float temperature, int apply_sigmoid, void *ref_in_dev,
                                float *ref_in32_dev, void *embed_dev);

/* ------------------------------------------------------------------------------------------
 * Token geometry of the deformable encoder / two-stage proposal head, one launch (f16 path).
 *
 * Replaces get_reference_points (codetr/transformer.py:280-305), reference_points[:, :, None] * valid_ratios[:, None]
 * (:530), make_encoder_output_proposals_export (:331-339) and the proposal half of
 * apply_mask_to_proposal_and_memory (:351-380); its memory half (`memory * total_mask`) is expressed as row
 * state 2 for codetr_linear_*'s row mask on enc_output.
 *
 *   valid_ratios_dev        [B, L, 2] f16 (w, h)
 *   mask_flat_dev           [B, S] uint8, non-zero = padding (codetr_mask_pyramid's output)
 *   level_shapes_host       HOST array of 2*L int64 (H_l, W_l)
 *   reference_points_dev    out [B, S, 2] f16 (x, y), the reference's own fp16 roundings: (x + .5) / f16(vr_w W_l)
 *                           rounded once.  The pixel centre x + .5 is exact (fp32); in fp16 so is the reference's
 *                           linspace up to 2048, but bf16 cannot hold a .5 centre from 128 up, so the bf16 twin is
 *                           NOT bit-equal to ATen's bf16 linspace formulation: it is the exact quotient rounded once,
 *                           never further from the fp32 result than that formulation.
 *   reference_by_level_dev  out [B, S, L, 2] f16
 *   proposals_dev           out [B, S, 4] f16: logit of (x, y, 0.05*2^l, 0.05*2^l) where the token is kept,
 *                           finfo(f16).max (NaN where the logit is not finite) where it is dropped
 *   row_state_dev           out [B, S] uint8: 0 = kept, 2 = dropped (padding, or a logit outside (-4.6, 4.6))
 * ------------------------------------------------------------------------------------------ */
int codetr_encoder_geometry_f16(void *stream, const void *valid_ratios_dev, const void *mask_flat_dev, int64_t B,
                                int num_levels, const int64_t *level_shapes_host, void *reference_points_dev,
                                void *reference_by_level_dev, void *proposals_dev, void *row_state_dev);
int codetr_encoder_geometry_bf16(void *stream, const void *valid_ratios_dev, const void *mask_flat_dev, int64_t B,
                                int num_levels, const int64_t *level_shapes_host, void *reference_points_dev,
                                void *reference_by_level_dev, void *proposals_dev, void *row_state_dev);

/* out[r] = max_c x[r, c] (NaN propagates, as torch.max): enc_outputs_class.max(-1)[0], the ranking score of
 * the two-stage top-k (codetr/transformer.py:560).  x [rows, C] f16 dense, out [rows] f16. */
int codetr_row_max_f16(void *stream, const void *x_dev, void *out_dev, int64_t rows, int64_t C);
int codetr_row_max_bf16(void *stream, const void *x_dev, void *out_dev, int64_t rows, int64_t C);

/* ------------------------------------------------------------------------------------------
 * Pre- and post-processing either side of CoDETR.forward (the reference's Inferencer, codetr/inferencer.py).
 *
 * codetr_preprocess_u8_*: one image, uint8 HWC RGB on the device -> normalised CHW in the model dtype + padding mask.
 *   Replaces the CPU test pipeline + DetDataPreprocessor + mask loop (codetr/inferencer.py:439-452, 354-358; configs
 *   co_dino_5scale_swin_l_16xb1_16e_o365tococo.py:88-96): mmdet Resize(keep_ratio) = cv2.resize(INTER_LINEAR) with
 *   OpenCV's 8-bit fixed-point arithmetic, Pad(size, pad_val) to the right / bottom, (x - mean) / std in fp32.
 *     src_dev            [H_src, W_src, 3] uint8
 *     H_resized/W_resized  size of the resized image (host: int(dim * factor + 0.5), mmcv.imrescale)
 *     H_pad/W_pad        output size (>= resized size)
 *     mean_host/std_host/pad_value_host   HOST arrays of 3 (per channel, in 0..255 units; pad value is a uint8 pixel
 *                        value that is normalised like the image, as Pad runs before the normalisation)
 *     dst_dev            [3, H_pad, W_pad]; mask_dev [H_pad, W_pad] (same dtype, 0 inside the image, 1 in the padding)
 *                        or NULL
 * codetr_batched_nms_f32: torchvision.ops.batched_nms of postprocess_predictions (codetr/inferencer.py:388-398):
 *   greedy per-class hard NMS, IoU > iou_threshold suppresses.  boxes_sorted_dev [N, 4] fp32 xyxy and
 *   labels_sorted_dev [N] int64 in DESCENDING SCORE ORDER; keep_dev [N] uint8 out (1 = kept).  One workgroup (N is
 *   <= 300 on this path; up to 60 000 accepted).
 * ------------------------------------------------------------------------------------------ */
int codetr_preprocess_u8_f16(void *stream, const void *src_dev, int64_t H_src, int64_t W_src, int64_t H_resized,
                             int64_t W_resized, int64_t H_pad, int64_t W_pad, const float *mean_host,
                             const float *std_host, const int *pad_value_host, void *dst_dev, void *mask_dev);
int codetr_preprocess_u8_f32(void *stream, const void *src_dev, int64_t H_src, int64_t W_src, int64_t H_resized,
                             int64_t W_resized, int64_t H_pad, int64_t W_pad, const float *mean_host,
                             const float *std_host, const int *pad_value_host, void *dst_dev, void *mask_dev);
int codetr_batched_nms_f32(void *stream, const float *boxes_sorted_dev, const int64_t *labels_sorted_dev, int64_t N,
                           float iou_threshold, void *keep_dev);

/* ------------------------------------------------------------------------------------------
 * Batched pre- and post-processing: the Inferencer's per-image steps (codetr/inferencer.py:343-400, 439-452) for a
 * chunk of images in one launch each.
 *
 * codetr_preprocess_batch_u8_*: up to CODETR_PREPROCESS_BATCH_MAX uint8 HWC RGB images of different sizes -> the
 *   stacked batch_inputs [N, 3, H, W] and img_masks [N, H, W] (dtype of the entry).  Per image the arithmetic of
 *   codetr_preprocess_u8_* (f16 / f32 results are bit-identical to it; bf16 is the f32 value rounded once), then
 *   DetDataPreprocessor's divisor padding + mmdet stack_batch: beyond the image's Pad region, up to (H, W), every
 *   value is pad_fill (as given, not normalised) and the mask is 1.
 *     src_dev            all images' bytes, src_bytes long; image n at byte offset images_host[7n]
 *     images_host        HOST [N][7] int64: src_offset, H_src, W_src, H_resized, W_resized, H_pad, W_pad
 *                        (H_resized <= H_pad <= H, W_resized <= W_pad <= W; the image must lie inside src)
 *     mean_host/std_host/pad_value_host   as codetr_preprocess_u8_*
 *     mask_dev           [N, H, W] or NULL
 *   The table travels in the kernel arguments: no staging copy, capturable.  CODETR_E_BADARG for null pointers,
 *   N <= 0 and inconsistent rows; CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX (the caller splits),
 *   H > 65535 or a source side > 32767.
 *
 * codetr_postprocess_detections_*: postprocess_predictions + the rescale of run_inference for N images of Q
 *   detections (boxes_dev [N, Q, 4] xyxy, scores_dev [N, Q] in T; labels_dev [N, Q] int64), one workgroup per image:
 *     1. apply_threshold: keep score > score_threshold compared at T's precision (the threshold rounded to T first,
 *        as `scores > thr` on a T tensor does); NaN scores fail it;
 *     2. apply_nms: stable descending sort of the survivors by score (torch.sort(scores.float(), descending=True,
 *        stable=True), a radix sort here: ties by ascending index, NaN first -- a NaN with the sign bit set last --,
 *        -0 equal to +0), then codetr_batched_nms_f32's greedy per-class NMS (same
 *        fp32 IoU arithmetic, IoU > iou_threshold suppresses); without NMS the survivors keep their index order;
 *     3. boxes / divisor_dev [N, 4] (T; the host's scale-factor tensor) in fp32, rounded once to T.
 *   Outputs, compacted per image: boxes_out_dev [N, Q, 4], scores_out_dev [N, Q] (T), labels_out_dev [N, Q] int64,
 *   count_dev [N] int32 = how many rows of image n are detections; the rows after them are zero.
 *   CODETR_E_BADARG for null pointers, N <= 0 or Q <= 0; CODETR_E_TOO_LARGE for Q > CODETR_POSTPROCESS_MAX_Q.
 *
 * codetr_postprocess_softnms_*: the post-processing the model configs specify -- test_cfg[0] =
 *   dict(max_per_img=300, nms=dict(type='soft_nms', iou_threshold=0.8)), configs/co_dino_5scale_r50_lsj_8xb2_1x_coco.py:80,
 *   inherited by all three configs -- i.e. mmcv 2.x batched_nms(..., nms_cfg=dict(type='soft_nms')) (methods linear and
 *   naive) followed by mmdet's results[:max_per_img], with the rescale of run_inference; same operands as
 *   codetr_postprocess_detections_*, one workgroup per image.  For image n with candidates (box_j, score_j, label_j),
 *   j the query index:
 *     1. boxes and scores convert to fp32 (exact); everything below is fp32 with one rounding per operation, and
 *        area_j = (x2 - x1) * (y2 - y1) is rounded once and stored;
 *     2. apply_threshold: as codetr_postprocess_detections_* (score > threshold at T's precision); a NaN score is
 *        dropped in this mode (a deviation: what mmcv does with a NaN is an accident of its scan order);
 *     3. g = the surviving candidate with the highest score (ties: lowest j); every candidate other than g whose score
 *        is < min_score is dropped (mmcv emits its first pick unchecked and tests all others in its first pass);
 *     4. per label, independently, while a candidate of the label is alive: pick the alive k with the highest current
 *        score (ties: lowest j), emit (k, current score), retire k; for every other alive j of the label
 *        w = max(0, min(x2) - max(x1)), h likewise, inter = w * h, ovr = inter / (area_k + area_j - inter);
 *        weight = (ovr >= iou_threshold) ? (method linear: 1 - ovr, naive: 0) : 1; s_j = s_j * weight; j is dropped if
 *        s_j < min_score.  A NaN ovr (two zero-area boxes) compares false: weight 1;
 *     5. the emitted detections are sorted by decayed score descending (ties: ascending j); the first max_keep stay
 *        (max_keep <= 0: all);
 *     6. boxes / divisor_dev in fp32 rounded once to T; the score is the decayed score rounded once to T.
 *   "Highest score" is the order of codetr_postprocess_detections_*'s sort: -0 equals +0, a NaN with the sign bit clear
 *   is above +inf, one with it set below -inf.  Two deliberate differences from mmcv: classes are separated by
 *   comparing labels, not by adding label * (max + 1) to the coordinates (as codetr_batched_nms_f32 already does; it
 *   also keeps the IoUs from being rounded at coordinates around 1.5e5), and ties go to the lowest query index rather
 *   than following mmcv's swap-with-last bookkeeping.  Method gaussian is not provided.
 *   Outputs as codetr_postprocess_detections_* plus index_out_dev [N, Q] int32, the query index of every output row.
 *   CODETR_E_BADARG for null pointers, N <= 0, Q <= 0, a method other than the two below, an iou_threshold or min_score
 *   that is not finite; CODETR_E_TOO_LARGE for Q > CODETR_POSTPROCESS_MAX_Q.  All checks run before any HIP call.
 * ------------------------------------------------------------------------------------------ */
#define CODETR_PREPROCESS_BATCH_MAX 32
#define CODETR_POSTPROCESS_MAX_Q 1024
int codetr_preprocess_batch_u8_f16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *images_host, int64_t H, int64_t W, const float *mean_host,
                                   const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                   void *mask_dev);
int codetr_preprocess_batch_u8_bf16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                    const int64_t *images_host, int64_t H, int64_t W, const float *mean_host,
                                    const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                    void *mask_dev);
int codetr_preprocess_batch_u8_f32(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *images_host, int64_t H, int64_t W, const float *mean_host,
                                   const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                   void *mask_dev);
int codetr_postprocess_detections_f16(void *stream, const void *boxes_dev, const void *scores_dev,
                                      const int64_t *labels_dev, const void *divisor_dev, int64_t N, int64_t Q,
                                      int apply_threshold, float score_threshold, int apply_nms, float iou_threshold,
                                      void *boxes_out_dev, void *scores_out_dev, int64_t *labels_out_dev,
                                      int *count_dev);
int codetr_postprocess_detections_bf16(void *stream, const void *boxes_dev, const void *scores_dev,
                                       const int64_t *labels_dev, const void *divisor_dev, int64_t N, int64_t Q,
                                       int apply_threshold, float score_threshold, int apply_nms, float iou_threshold,
                                       void *boxes_out_dev, void *scores_out_dev, int64_t *labels_out_dev,
                                       int *count_dev);
int codetr_postprocess_detections_f32(void *stream, const void *boxes_dev, const void *scores_dev,
                                      const int64_t *labels_dev, const void *divisor_dev, int64_t N, int64_t Q,
                                      int apply_threshold, float score_threshold, int apply_nms, float iou_threshold,
                                      void *boxes_out_dev, void *scores_out_dev, int64_t *labels_out_dev,
                                      int *count_dev);
#define CODETR_SOFTNMS_NAIVE 0
#define CODETR_SOFTNMS_LINEAR 1
int codetr_postprocess_softnms_f16(void *stream, const void *boxes_dev, const void *scores_dev,
                                   const int64_t *labels_dev, const void *divisor_dev, int64_t N, int64_t Q,
                                   int apply_threshold, float score_threshold, int method, float iou_threshold,
                                   float min_score, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                                   int64_t *labels_out_dev, int *index_out_dev, int *count_dev);
int codetr_postprocess_softnms_bf16(void *stream, const void *boxes_dev, const void *scores_dev,
                                    const int64_t *labels_dev, const void *divisor_dev, int64_t N, int64_t Q,
                                    int apply_threshold, float score_threshold, int method, float iou_threshold,
                                    float min_score, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                                    int64_t *labels_out_dev, int *index_out_dev, int *count_dev);
int codetr_postprocess_softnms_f32(void *stream, const void *boxes_dev, const void *scores_dev,
                                   const int64_t *labels_dev, const void *divisor_dev, int64_t N, int64_t Q,
                                   int apply_threshold, float score_threshold, int method, float iou_threshold,
                                   float min_score, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                                   int64_t *labels_out_dev, int *index_out_dev, int *count_dev);

/* ------------------------------------------------------------------------------------------
 * Test-time augmentation (mmdet 3.x DetTTAModel + the TestTimeAug pipeline): one image as several views -- scales,
 * horizontal flip -- and the fusion of the views' detections, both on the device.
 *
 * codetr_preprocess_views_u8_*: codetr_preprocess_batch_u8_* with one more column per row,
 *     images_host        HOST [N][8] int64: src_offset, H_src, W_src, H_resized, W_resized, H_pad, W_pad, flip
 *   A row with flip = 1 holds the resized image mirrored left to right inside its resized width: output column
 *   x < W_resized is what column W_resized - 1 - x is with flip = 0 (mmdet's RandomFlip runs after Resize and before any
 *   padding, so the padding stays on the right).  The Pad region beyond the image, the divisor padding, pad_fill and the
 *   mask are those of flip = 0.  Rows may name the same src_offset: several views read one uploaded image.  A flip
 *   other than 0 or 1 is CODETR_E_BADARG; every other limit and error code is codetr_preprocess_batch_u8_*'s.
 *
 * codetr_tta_merge_*: DetTTAModel._merge_single_sample -- un-flip, concatenate, batched_nms(tta_cfg.nms), cut to
 *   max_per_img -- for N images of V views, one workgroup per image.  The operands are the stacked outputs of the
 *   per-view codetr_postprocess_* launches, already in original-image coordinates:
 *     boxes_dev [V, N, Q, 4], scores_dev [V, N, Q] in T; labels_dev [V, N, Q] int64; count_dev [V, N] int32: rows
 *     j < count[v, n] of view v are image n's candidates; flip_mask: bit v set = view v was flipped; width_dev [N]
 *     fp32: the original image width W.  The candidate index is c = v * Q + j.
 *     1. boxes and scores convert to fp32 (exact); a flipped view's box becomes (W - x2, y1, W - x1, y2), one fp32
 *        rounding per coordinate; everything below is fp32 with one rounding per operation, never contracted, and
 *        area_c = (x2 - x1) * (y2 - y1) is one rounded product (steps 1 and 4 of codetr_postprocess_softnms_*: the same
 *        ovr = inter / (area_k + area_c - inter));
 *     2. "highest score" is codetr_postprocess_detections_*'s order (-0 equals +0, NaN with the sign bit clear above
 *        +inf); ties go to the lowest c;
 *     3. mode CODETR_TTA_NMS_HARD, per label, while a candidate of the label is alive: pick the alive k with the
 *        highest score, emit (k, score_k), retire k and every alive c of the label with ovr > iou_threshold (a NaN ovr
 *        compares false).  min_score is not used;
 *        modes CODETR_TTA_NMS_SOFT_NAIVE / _SOFT_LINEAR: steps 3 to 5 of codetr_postprocess_softnms_* over the
 *        concatenated candidates (the min_score drop that spares the global maximum, the per-label decay chains);
 *     4. the emitted detections are sorted by (decayed) score descending, ties by ascending c; the first max_keep stay
 *        (max_keep <= 0: all).
 *   Outputs, K = max_keep (V * Q when max_keep <= 0): boxes_out_dev [N, K, 4], scores_out_dev [N, K] in T (the fp32
 *   value rounded once), labels_out_dev [N, K] int64, index_out_dev [N, K] int32 = the c of every row, count_out_dev [N]
 *   int32; rows beyond count_out[n] are zero.  Parity with mmdet / mmcv is unpinned (neither is installed where this is
 *   tested); the deviations are those of codetr_postprocess_softnms_*: labels are compared instead of offsetting the
 *   coordinates, ties go to the lowest index, and the IoU arithmetic is this library's.
 *   The workgroup keeps all candidates in LDS (36 bytes per slot of the power of two >= V * Q, 144 KB at 4096): no
 *   workspace operand.  CODETR_E_BADARG for a null pointer, V, N or Q <= 0, a flip bit at or above V, a mode other than
 *   the three below, an iou_threshold or min_score that is not finite; CODETR_E_TOO_LARGE for V > CODETR_TTA_MAX_VIEWS
 *   or V * Q > CODETR_TTA_MAX_CANDIDATES.  All checks run before any HIP call.
 * ------------------------------------------------------------------------------------------ */
#define CODETR_TTA_MAX_VIEWS 16
#define CODETR_TTA_MAX_CANDIDATES 4096
#define CODETR_TTA_NMS_HARD 0
#define CODETR_TTA_NMS_SOFT_NAIVE 1
#define CODETR_TTA_NMS_SOFT_LINEAR 2
int codetr_preprocess_views_u8_f16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *images_host, int64_t H, int64_t W, const float *mean_host,
                                   const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                   void *mask_dev);
int codetr_preprocess_views_u8_bf16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                    const int64_t *images_host, int64_t H, int64_t W, const float *mean_host,
                                    const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                    void *mask_dev);
int codetr_preprocess_views_u8_f32(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *images_host, int64_t H, int64_t W, const float *mean_host,
                                   const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                   void *mask_dev);
int codetr_tta_merge_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                         const int *count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask,
                         const float *width_dev, int mode, float iou_threshold, float min_score, int64_t max_keep,
                         void *boxes_out_dev, void *scores_out_dev, int64_t *labels_out_dev, int *index_out_dev,
                         int *count_out_dev);
int codetr_tta_merge_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                          const int *count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask,
                          const float *width_dev, int mode, float iou_threshold, float min_score, int64_t max_keep,
                          void *boxes_out_dev, void *scores_out_dev, int64_t *labels_out_dev, int *index_out_dev,
                          int *count_out_dev);
int codetr_tta_merge_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                         const int *count_dev, int64_t V, int64_t N, int64_t Q, uint32_t flip_mask,
                         const float *width_dev, int mode, float iou_threshold, float min_score, int64_t max_keep,
                         void *boxes_out_dev, void *scores_out_dev, int64_t *labels_out_dev, int *index_out_dev,
                         int *count_out_dev);

/* ------------------------------------------------------------------------------------------
 * Sliced inference (SAHI's slicing, beyond the reference): one image as overlapping tiles, each run as an image of its
 * own, optionally next to the whole image, and the fusion of their detections, both on the device.
 *
 * codetr_preprocess_tiles_u8_*: codetr_preprocess_batch_u8_* with a crop rectangle per row,
 *     tiles_host         HOST [N][11] int64: src_offset, H_img, W_img, y0, x0, H_crop, W_crop, H_resized, W_resized,
 *                        H_pad, W_pad
 *   A row's source is the H_crop x W_crop window whose top-left pixel is (y0, x0) of the H_img x W_img image at
 *   src_offset (its rows W_img * 3 bytes apart).  The output row is, bit for bit, what codetr_preprocess_batch_u8_* writes
 *   for a contiguous copy of that window: the resize coefficients come from the crop's size, the sy + 1 / sx + 1
 *   neighbour is clamped to the crop (a pixel outside it is never read), and the Pad region, the divisor padding, pad_fill
 *   and the mask are the batch entry's.  Rows may name the same src_offset: the tiles of an image read its one uploaded
 *   copy.  Limits and error codes are codetr_preprocess_batch_u8_*'s, with the side limit on H_img and W_img, plus
 *   CODETR_E_BADARG for y0 < 0, x0 < 0, H_crop <= 0, W_crop <= 0, y0 + H_crop > H_img or x0 + W_crop > W_img.  All checks
 *   run before any HIP call.
 *
 * codetr_slice_merge_*: the fusion of the views' detections (SAHI's postprocess: greedy NMS or greedy non-maximum
 *   merging, under IoU or IoS) for N images of up to V views, one workgroup per image.  The operands are the stacked
 *   outputs of the per-row codetr_postprocess_* launches, in each crop's own pixel coordinates:
 *     boxes_dev [R, Q, 4], scores_dev [R, Q] in T; labels_dev [R, Q] int64; count_dev [R] int32: rows j < count[r] of
 *     row r are candidates; rows_dev [N, V] int32: the row of image n's v-th view, a value outside [0, R) = the view is
 *     absent; origin_dev [R, 2] fp32: (x0, y0) of row r's crop in its image; size_dev [N, 2] fp32: (W, H) of the
 *     original image.  The candidate index is c = v * Q + j.  Everything below is fp32 with one rounding per
 *     operation, never contracted.
 *     1. boxes and scores convert to fp32 (exact); each coordinate gets + x0 or + y0 (one rounding) and is clipped to
 *        the image with fminf(fmaxf(v, 0), W or H) -- a NaN coordinate becomes 0; area_c = (x2 - x1) * (y2 - y1) of the
 *        clipped box, one rounded product;
 *     2. "highest score" and ties are codetr_tta_merge_*'s: -0 equals +0, a NaN with the sign bit clear above +inf; ties
 *        go to the lowest c;
 *     3. the overlap of pick k and candidate c: w = max(0, min(x2) - max(x1)), h likewise, inter = w * h, then
 *        metric CODETR_SLICE_IOU: inter / (area_k + area_c - inter), codetr_postprocess_softnms_*'s ovr;
 *        metric CODETR_SLICE_IOS: inter / fminf(area_k, area_c), the intersection over the smaller area.
 *        A NaN overlap (0 / 0: a box of no area) compares false;
 *     4. segments: the candidates of one label; with class_agnostic != 0 all candidates of the image form one segment;
 *     5. mode CODETR_SLICE_NMS, per segment, while a candidate of it is alive: pick the alive k with the highest score,
 *        emit (box_k, score_k, label_k), retire k and every alive c of the segment with overlap > threshold;
 *     6. mode CODETR_SLICE_NMM (greedy non-maximum merging): the same pick and the same retirement, but the retired c
 *        are absorbed: the emitted box is (min x1, min y1, max x2, max y2) over k and the boxes it absorbed -- min and
 *        max only, hence exact and free of any order --, the emitted score and label are k's.  Overlaps are always
 *        measured against k's original box, never a grown one, and an absorbed box absorbs nothing itself;
 *     7. the emitted detections are sorted by score descending, ties by ascending c; the first max_keep stay
 *        (max_keep <= 0: all).
 *   Outputs exactly as codetr_tta_merge_*, K = max_keep (V * Q when max_keep <= 0): boxes_out_dev [N, K, 4],
 *   scores_out_dev [N, K] in T (rounded once), labels_out_dev [N, K] int64, index_out_dev [N, K] int32 = the c of every
 *   row (in NMM mode the c of the pick), count_out_dev [N] int32; rows beyond count_out[n] are zero.  Parity with SAHI is
 *   unpinned (it is not installed where this is tested); ties, label comparison and the overlap arithmetic are this
 *   library's, and SAHI's non-greedy NMM variant is not provided.
 *   LDS as codetr_tta_merge_* (36 bytes per slot of the power of two >= V * Q): no workspace operand.  CODETR_E_BADARG
 *   for a null pointer, R, N, V or Q <= 0, a metric or mode other than those below, a threshold that is not finite;
 *   CODETR_E_TOO_LARGE for V > CODETR_SLICE_MAX_VIEWS or V * Q > CODETR_TTA_MAX_CANDIDATES.  All checks run before any
 *   HIP call.
 * ------------------------------------------------------------------------------------------ */
#define CODETR_SLICE_MAX_VIEWS 64
#define CODETR_SLICE_IOU 0
#define CODETR_SLICE_IOS 1
#define CODETR_SLICE_NMS 0
#define CODETR_SLICE_NMM 1
int codetr_preprocess_tiles_u8_f16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *tiles_host, int64_t H, int64_t W, const float *mean_host,
                                   const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                   void *mask_dev);
int codetr_preprocess_tiles_u8_bf16(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *tiles_host, int64_t H, int64_t W, const float *mean_host,
                                   const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                   void *mask_dev);
int codetr_preprocess_tiles_u8_f32(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                                   const int64_t *tiles_host, int64_t H, int64_t W, const float *mean_host,
                                   const float *std_host, const int *pad_value_host, float pad_fill, void *dst_dev,
                                   void *mask_dev);
int codetr_slice_merge_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                           const int *count_dev, const int *rows_dev, const float *origin_dev, const float *size_dev,
                           int64_t R, int64_t N, int64_t V, int64_t Q, int metric, int mode, float threshold,
                           int class_agnostic, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                           int64_t *labels_out_dev, int *index_out_dev, int *count_out_dev);
int codetr_slice_merge_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                           const int *count_dev, const int *rows_dev, const float *origin_dev, const float *size_dev,
                           int64_t R, int64_t N, int64_t V, int64_t Q, int metric, int mode, float threshold,
                           int class_agnostic, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                           int64_t *labels_out_dev, int *index_out_dev, int *count_out_dev);
int codetr_slice_merge_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                           const int *count_dev, const int *rows_dev, const float *origin_dev, const float *size_dev,
                           int64_t R, int64_t N, int64_t V, int64_t Q, int metric, int mode, float threshold,
                           int class_agnostic, int64_t max_keep, void *boxes_out_dev, void *scores_out_dev,
                           int64_t *labels_out_dev, int *index_out_dev, int *count_out_dev);

/* ------------------------------------------------------------------------------------------
 * Visualisation: the predictions drawn on the original images, in place, one launch for a chunk.
 *
 * Replaces DetLocalVisualizer.add_datasample / _draw_instances as the reference's Inferencer.visualize drives them
 * (codetr/inferencer.py:163-235; the call at :458-470): per detection above pred_score_thr a box outline in the colour of
 * its class and, on a dark patch at the box's top-left corner, "<class name>: <score in percent>".  mmdet rasterises
 * through matplotlib; this library defines its own rendering, modelled on DetLocalVisualizer's defaults (line_width 3,
 * alpha 0.8, text colour (200, 200, 200), all boxes first and all texts after them, a text size that grows with the box
 * area), and states it here in integer pixel arithmetic.  Parity with mmdet's visualiser is unpinned (neither mmdet nor
 * matplotlib is installed where this is tested).
 *
 * codetr_draw_detections_*: N <= CODETR_PREPROCESS_BATCH_MAX images (the caller splits).
 *   Inputs, per image n:
 *     buf_dev            one flat byte buffer, buf_bytes long; image n is RGB uint8 HWC at byte offset images_host[3n],
 *                        images_host HOST [N][3] int64: offset, H, W; 1 <= H, W <= CODETR_DRAW_MAX_SIDE; the images must
 *                        lie inside the buffer and must not overlap.  No alignment is asked of offsets or row pitches.
 *     boxes_dev [N, Q, 4] xyxy in original-image coordinates, scores_dev [N, Q] in T; labels_dev [N, Q] int64;
 *     count_dev [N] int32: rows j < count[n] (clamped to 0..Q) are image n's detections, in the order the
 *                        post-processing kernels emit them; Q <= CODETR_DRAW_MAX_Q.
 *   Style: line_width lw in 1..15; alpha in [0, 1], A = (int)(alpha * 256.0f + 0.5f) in 0..256 (fp32); score_thr (fp32);
 *     text_rgb = 0xRRGGBB; font_scale in 1..4; draw_labels 0 / 1.
 *   Tables: palette_dev [C, 3] uint8; names_dev [C, 24] bytes: byte 0 of a row is the name's length <= 23, bytes 1.. are
 *     ASCII 32..126 (a longer length reads as 23, any other byte draws as '?').
 *   Drawn set: row j is drawn when its score widened to fp32 is > score_thr (strict; a NaN fails), its label is in
 *     [0, C), its four coordinates are finite and, with every coordinate clamped in fp32 to [-16384, 16383] and
 *     xi = (int)floorf(x + 0.5f) (one fp32 rounding in the sum), x2i >= x1i and y2i >= y1i.
 *   blend(p, c) = (p * (256 - A) + c * A + 128) >> 8 per channel.
 *   Layer 1, box edges, for j ascending: with a = lw / 2 and b = (lw - 1) / 2 (integer divisions), pixel (x, y) is on j's
 *     edge iff it lies in [x1i - a, x2i + a] x [y1i - a, y2i + a] and not in [x1i + b + 1, x2i - b - 1] x
 *     [y1i + b + 1, y2i - b - 1] (an empty inner rectangle: the box is filled); an edge pixel p becomes
 *     blend(p, palette[label]).
 *   Layer 2, labels, after every edge of the image, for j ascending (draw_labels = 1):
 *     text = names[label] + ": " + score text.  v = score * 1000.0f + 0.5f with one fp32 rounding after the multiply and
 *     one after the add (never an fma); n = 0 if !(v > 0), 1000 if v >= 1000, else (int)v; the score text is the decimal
 *     of n / 10, ".", the digit n % 10: 87.3, 5.0, 100.0.
 *     s = font_scale * (1 + ((x2i - x1i) * (y2i - y1i) >= 15400)): 15400 is the midpoint of mmdet's 800..30000 ramp.
 *     The text grid has 6 * len + 1 columns and 9 rows of font pixels, each s x s image pixels, its top-left image pixel
 *     at (x1i + lw, y1i + lw); character k fills grid columns 1 + 6k .. 5 + 6k and rows 1..7 from the 5x7 font below.
 *     A grid pixel whose font bit is set becomes text_rgb, opaque; every other grid pixel p becomes blend(p, black).
 *   Everything is clipped to the image; nothing is shifted or wrapped.  A pixel is written only if a layer changed it.
 *   One 256-thread workgroup per 64x16 tile (csrc/draw.hip); no workspace.  CODETR_E_BADARG for a null pointer, N, Q or
 *   C <= 0, an inconsistent row, a style value outside its range, a NaN score_thr; CODETR_E_TOO_LARGE for
 *   N > CODETR_PREPROCESS_BATCH_MAX, Q > CODETR_DRAW_MAX_Q, a side > CODETR_DRAW_MAX_SIDE, C > 65536.  All checks run
 *   before any HIP call.
 *
 * codetr_draw_font: HOST only -- copies the library's 5x7 font (authored for this library) to out_host: 95 glyphs, ASCII
 *   32..126, 7 bytes each, top row first; bit 4 of a byte is the leftmost of the row's 5 pixels, bits 5..7 are zero.
 *   The kernel reads the same table from __constant__ memory.  Returns 0, CODETR_E_BADARG for a null pointer.
 * ------------------------------------------------------------------------------------------ */
#define CODETR_DRAW_MAX_Q 4096
#define CODETR_DRAW_MAX_SIDE 16384
#define CODETR_DRAW_FONT_BYTES 665
int codetr_draw_font(unsigned char *out_host);
int codetr_draw_detections_f16(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                               const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                               const int *count_dev, int64_t Q, const unsigned char *palette_dev,
                               const unsigned char *names_dev, int64_t C, int line_width, float alpha, float score_thr,
                               uint32_t text_rgb, int font_scale, int draw_labels);
int codetr_draw_detections_bf16(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                                const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                                const int *count_dev, int64_t Q, const unsigned char *palette_dev,
                                const unsigned char *names_dev, int64_t C, int line_width, float alpha, float score_thr,
                                uint32_t text_rgb, int font_scale, int draw_labels);
int codetr_draw_detections_f32(void *stream, void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                               const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                               const int *count_dev, int64_t Q, const unsigned char *palette_dev,
                               const unsigned char *names_dev, int64_t C, int line_width, float alpha, float score_thr,
                               uint32_t text_rgb, int font_scale, int draw_labels);

/* ------------------------------------------------------------------------------------------
 * Frames: what decoders and capture libraries hand out -> the packed RGB images the kernels above read, one launch for a
 * chunk.  Beyond the reference, whose Inferencer takes host RGB arrays only (codetr/inferencer.py:402-452).
 *
 * codetr_frames_to_rgb_u8: N <= CODETR_PREPROCESS_BATCH_MAX frames (the caller splits).
 *     src_dev            one flat byte buffer, src_bytes long, holding every plane of every frame
 *     frames_host        HOST [N][10] int64: format, H, W, plane0_offset, plane0_pitch, plane1_offset, plane1_pitch,
 *                        plane2_offset, plane2_pitch, dst_offset.  Offsets are bytes from src_dev (dst_offset: from
 *                        dst_dev), a pitch is the distance in bytes between two rows of its plane and is at least the
 *                        row's bytes; the columns of a plane the format does not have are 0 and never read.
 *     dst_dev            dst_bytes long; frame n becomes RGB uint8 HWC, H * W * 3 bytes at dst_offset, its rows W * 3 bytes
 *                        apart (the layout codetr_preprocess_batch_u8_* and codetr_draw_detections_* take)
 *   Formats (ch = ceil(H / 2), cw = ceil(W / 2); odd H and W are allowed):
 *     CODETR_FRAME_RGB  0   one plane, H rows of 3 W bytes: R, G, B.  With a pitch: a pitched-to-packed copy
 *     CODETR_FRAME_BGR  1   one plane, H rows of 3 W bytes: B, G, R
 *     CODETR_FRAME_RGBA 2   one plane, H rows of 4 W bytes: R, G, B, A; alpha is ignored
 *     CODETR_FRAME_BGRA 3   one plane, H rows of 4 W bytes: B, G, R, A; alpha is ignored
 *     CODETR_FRAME_GRAY 4   one plane, H rows of W bytes; R = G = B = the byte, no range expansion
 *     CODETR_FRAME_NV12 5   plane 0: Y, H rows of W bytes; plane 1: ch rows of cw interleaved pairs U, V (2 cw bytes)
 *     CODETR_FRAME_NV21 6   as NV12, the pairs V, U
 *     CODETR_FRAME_I420 7   plane 0: Y; plane 1: U, ch rows of cw bytes; plane 2: V, the same shape
 *   Chroma is taken nearest: pixel (y, x) uses chroma sample (y >> 1, x >> 1), as OpenCV's
 *   cvtColor(..., COLOR_YUV2RGB_NV12) does.
 *   YUV -> RGB, per launch a matrix (CODETR_COLOR_BT601 0, CODETR_COLOR_BT709 1) and a range (CODETR_COLOR_LIMITED 0,
 *   CODETR_COLOR_FULL 1).  With c = max(0, Y - y0), d = U - 128, e = V - 128, y0 = 16 for limited and 0 for full range:
 *       R = clamp255((CY * c           + CRV * e + (1 << 19)) >> 20)
 *       G = clamp255((CY * c + CGU * d + CGV * e + (1 << 19)) >> 20)
 *       B = clamp255((CY * c + CBU * d           + (1 << 19)) >> 20)
 *   in signed 32-bit arithmetic (the largest magnitude is below 2^30), >> an arithmetic shift, clamp255 to 0..255.
 *   The constants are round(k * 2^20), {CY, CRV, CGU, CGV, CBU} below.  BT.601 limited takes OpenCV's published
 *   three-decimal coefficients k = 1.164, 1.596, -0.391, -0.813, 2.018 -- the default, because it is what a caller's
 *   cvtColor does today.  The other three sets come from the exact matrices evaluated in double: with (Kr, Kb) =
 *   (0.299, 0.114) for BT.601 and (0.2126, 0.0722) for BT.709 and Kg = 1 - Kr - Kb, full range is CY = 1, CRV = 2 (1 - Kr),
 *   CBU = 2 (1 - Kb), CGU = -2 Kb (1 - Kb) / Kg, CGV = -2 Kr (1 - Kr) / Kg; limited range multiplies CY by 255 / 219 and
 *   the chroma terms by 255 / 224.  Parity with OpenCV is unpinned (cv2 is not installed where this is tested): the
 *   formula above is the contract.
 *   Reads: no byte outside a declared plane row [offset + r * pitch, offset + r * pitch + row bytes) is read, by a
 *   vector load either; whatever lies between the rows of a pitched plane does not matter.  Writes: no byte outside an
 *   output image is written.  Offsets and pitches need no alignment; rows whose addresses are multiples of 4 move as
 *   dwords (csrc/frames.hip) with the same result.
 *   The table travels in the kernel arguments: no staging copy, capturable.  CODETR_E_BADARG for a null pointer,
 *   N <= 0, src_bytes or dst_bytes <= 0, an unknown format, matrix or range, H or W <= 0, a negative offset, a pitch
 *   smaller than the row's bytes, a plane row not inside [0, src_bytes), an output image not inside [0, dst_bytes), two
 *   output images that overlap; CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX or a side above
 *   CODETR_FRAME_MAX_SIDE (the source-side limit of codetr_preprocess_batch_u8_*).  All checks run before any HIP call.
 * ------------------------------------------------------------------------------------------ */
#define CODETR_FRAME_RGB 0
#define CODETR_FRAME_BGR 1
#define CODETR_FRAME_RGBA 2
#define CODETR_FRAME_BGRA 3
#define CODETR_FRAME_GRAY 4
#define CODETR_FRAME_NV12 5
#define CODETR_FRAME_NV21 6
#define CODETR_FRAME_I420 7
#define CODETR_FRAME_MAX_SIDE 32767
#define CODETR_COLOR_BT601 0
#define CODETR_COLOR_BT709 1
#define CODETR_COLOR_LIMITED 0
#define CODETR_COLOR_FULL 1
/*                                   CY       CRV      CGU      CGV      CBU  */
#define CODETR_YUV_BT601_LIMITED {1220542, 1673527, -409993, -852492, 2116026}
#define CODETR_YUV_BT601_FULL    {1048576, 1470104, -360853, -748826, 1858077}
#define CODETR_YUV_BT709_LIMITED {1220945, 1879825, -223607, -558796, 2215014}
#define CODETR_YUV_BT709_FULL    {1048576, 1651297, -196424, -490864, 1945738}
int codetr_frames_to_rgb_u8(void *stream, const void *src_dev, int64_t src_bytes, int64_t N,
                            const int64_t *frames_host, int matrix, int range, void *dst_dev, int64_t dst_bytes);

/* ------------------------------------------------------------------------------------------
 * Tracking: track ids for the detections of consecutive frames, association and Kalman filtering in one launch per chunk,
 * the state of every stream (camera) kept on the device.  Beyond the reference, whose Inferencer treats every image as
 * unrelated.  The rule is modelled on mmdet 3.x ByteTracker with its KalmanFilter and is this library's own where stated;
 * parity with mmdet is unpinned (mmdet is not installed where this is tested): the text below is the contract.
 *
 * codetr_track_update_{f16,bf16,f32}: N <= CODETR_PREPROCESS_BATCH_MAX rows (frames) of Q <= CODETR_POSTPROCESS_MAX_Q
 * detections, exactly the (boxes [N,Q,4], scores [N,Q], labels [N,Q] int64, count [N] int32) a
 * codetr_postprocess_detections_* / _softnms_* / codetr_tta_merge_* / codetr_slice_merge_* launch wrote.
 *     stream_of_row_host  HOST [N] int: the stream s in [0, S) every row belongs to.  The rows of one stream are its
 *                         consecutive frames in row order; they are walked in that order inside the one launch (one
 *                         workgroup per stream).  The table travels in the kernel arguments: no staging copy, capturable.
 *     state_dev           [S] states of codetr_track_state_bytes(max_tracks) bytes each, read and written back once per
 *                         launch; the state of a stream without a row is not touched.  A zero-filled state is a fresh
 *                         stream.  8-byte aligned.
 *     settings_host       HOST [6] float: obj_score_thrs.high, obj_score_thrs.low, init_track_thr, match_iou_thrs.high,
 *                         match_iou_thrs.low, match_iou_thrs.tentative
 *     retain, tentatives  num_frames_retain, num_tentatives (>= 1); weight_iou: weight_iou_with_det_scores (0 / 1)
 *     track_id_out_dev    [N, Q] int32, every element written: the id of the track a row updated or started, negated
 *                         while that track is tentative, 0 for no track and for rows >= count[n]
 *   This build's defaults (mmdet's ByteTracker config values as recalled; they cannot be checked where mmdet is absent):
 *   obj_score_thrs high 0.6 low 0.1, init_track_thr 0.7, weight_iou_with_det_scores on, match_iou_thrs high 0.1 low 0.5
 *   tentative 0.3, num_frames_retain 30, num_tentatives 3; max_tracks 256 is this build's own.
 *
 *   State of a stream with T = max_tracks slots, 16 + 104 T bytes, a struct of arrays in this order:
 *       int32 f, issued, refused, 0      the frame counter, the ids given out so far (next_id = issued + 1: ids start at
 *                                        1), the track starts refused for lack of a free slot
 *       int64 label[T]
 *       int32 id[T]                      0: the slot is free, and then every other field of the slot is 0
 *       int32 hits[T], tentative[T], last[T]     frames matched, 1 while tentative, the frame of the last match
 *       float mean[8][T]                 row 2 c + i: coordinate c of (cx, cy, a = w / h, h), i = 0 position p, 1 velocity v
 *       float cov[12][T]                 row 3 c + i: coordinate c, i = 0, 1, 2 the A, B, C of its covariance [[A, B], [B, C]]
 *
 *   Arithmetic: fp32, one rounding per operation in the order written (nothing is contracted into an FMA), divisions are
 *   IEEE.  Boxes and scores are widened to fp32 exactly.  wp = 1.0f / 20.0f, wv = 1.0f / 160.0f.
 *   The filter: mmdet's 8x8 Kalman filter has diagonal noise and initial covariance and a constant-velocity transition,
 *   so it is exactly four independent two-state filters, one per coordinate.  For coordinate c at height h the position
 *   standard deviation is s_p = wp * h (c = a: 1e-2f), the velocity standard deviation s_v = wv * h (a: 1e-5f).
 *     initiate from z = (cx, cy, a, h):  p = z_c, v = 0, B = 0;  t = 2.0f * (wp * z_h), A = t * t;
 *                         u = 10.0f * (wv * z_h), C = u * u;  for a: A = 1e-2f * 1e-2f, C = 1e-5f * 1e-5f
 *     predict (h = the p of coordinate h before the step, the same h for all four coordinates):
 *                         p' = p + v;  A' = ((A + 2.0f * B) + C) + s_p * s_p;  B' = B + C;  C' = C + s_v * s_v
 *     update with z (h = the predicted p of coordinate h, read before any coordinate is updated): r = s_p * s_p
 *                         (a: 1e-1f * 1e-1f);  S = A + r;  k0 = A / S;  k1 = B / S;  y = z_c - p;
 *                         p' = p + k0 * y;  v' = v + k1 * y;  A' = A - k0 * A;  B' = B - k0 * B;  C' = C - k1 * B
 *   A detection's measurement: cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f, h = y2 - y1, a = (x2 - x1) / h.
 *   A track's box: w = a * h, hw = w * 0.5f, hh = h * 0.5f, (cx - hw, cy - hh, cx + hw, cy + hh) of the predicted mean.
 *   Overlap of a track's box k and a candidate c: the IoU of the soft-NMS kernel above -- area = (x2 - x1) * (y2 - y1) of
 *   the box's corners, one rounded product; iw = max(0, min(x2k, x2c) - max(x1k, x1c)), ih likewise, inter = iw * ih,
 *   inter / ((area_k + area_c) - inter).  A NaN overlap or value compares false: the pair is not eligible.
 *
 *   Per frame (row) of a stream, in this order, f the stream's frame counter:
 *   1. Candidates are rows j < clamp(count[n], 0, Q).  A row with a non-finite coordinate or score, x2 - x1 <= 0 or
 *      y2 - y1 <= 0 takes no part and gets id 0.  `high`: score > obj high;  `low`: obj low < score <= obj high.
 *   2. Every live track with last != f - 1 gets the v of coordinate h set to 0; then every live track is predicted.
 *   3. Match A: the confirmed (not tentative) tracks, lost ones included, against the high candidates.  The value of a
 *      pair is iou * score (one rounded product) with weight_iou, else iou; the pair is eligible when the labels are
 *      equal (classes are told apart by comparing labels, as everywhere in this library) and value >= match high.
 *      The matching is GREEDY: repeatedly the eligible pair of the highest value among the tracks and candidates not yet
 *      matched is taken, ties to the lowest slot, then the lowest j.  (mmdet solves an assignment problem with `lap`;
 *      greedy is this library's deliberate deviation, as ties and label comparison are.)
 *   4. Match B: the tentative tracks against the high candidates still free, the same value, threshold match tentative.
 *   5. Match C: the confirmed tracks still unmatched with last == f - 1 against the low candidates; the value is plain
 *      iou, never weighted; threshold match low.
 *   6. Every matched track: the filter update with its candidate's measurement; last = f, hits += 1, the label becomes the
 *      candidate's; a tentative track is confirmed once hits >= num_tentatives.
 *   7. An unmatched tentative track is freed; an unmatched confirmed track with f - last >= num_frames_retain is freed.
 *   8. The free high candidates with score > init_track_thr start tracks, in ascending j, each in the lowest free slot
 *      (slots freed in step 7 included): id = ++issued, hits = 1, last = f, the candidate's label, the filter initiated
 *      from its measurement; confirmed when f == 0, tentative otherwise.  Without a free slot the candidate gets id 0 and
 *      `refused` goes up by one.
 *   9. Output as described at track_id_out_dev (the track's state after this frame decides the sign); then f += 1.
 *
 * codetr_track_state_bytes: host only; 16 + 104 max_tracks, CODETR_E_BADARG outside [1, CODETR_TRACK_MAX_TRACKS].
 * CODETR_E_BADARG for a null pointer, N, Q, S or max_tracks <= 0, a stream index outside [0, S), a setting that is not
 * finite, retain or tentatives < 1; CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX, Q > CODETR_POSTPROCESS_MAX_Q
 * or max_tracks > CODETR_TRACK_MAX_TRACKS.  All checks run before any HIP call.
 * ------------------------------------------------------------------------------------------ */
#define CODETR_TRACK_MAX_TRACKS 512
int64_t codetr_track_state_bytes(int64_t max_tracks);
int codetr_track_update_f16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                            const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                            void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                            int64_t tentatives, int weight_iou, int *track_id_out_dev);
int codetr_track_update_bf16(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                             const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                             void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                             int64_t tentatives, int weight_iou, int *track_id_out_dev);
int codetr_track_update_f32(void *stream, const void *boxes_dev, const void *scores_dev, const int64_t *labels_dev,
                            const int *count_dev, int64_t N, int64_t Q, const int *stream_of_row_host, int64_t S,
                            void *state_dev, int64_t max_tracks, const float *settings_host, int64_t retain,
                            int64_t tentatives, int weight_iou, int *track_id_out_dev);

/* ------------------------------------------------------------------------------------------
 * Backward of multi-scale deformable attention (training path).
 *
 * Replaces ms_deformable_col2im_cuda<T> / ms_deform_attn_backward (codetr/csrc/ms_deform_attn.cu:781-897, 975-1028;
 * arithmetic of ms_deform_attn_col2im_bilinear :79-146): same operands as the forward plus
 *   grad_output_dev        [B, Nq, M*D]          T
 *   grad_value_dev         [B, S, M, D]          T   accumulated with atomics -- the CALLER zero-fills all three
 *   grad_sampling_loc_dev  [B, Nq, M, L, P, 2]   T   gradients first (reference codetr/ops.py:94-96)
 *   grad_attn_weight_dev   [B, Nq, M, L, P]      T
 * T in {f16, f32, f64}; f16 computes in fp32 and accumulates grad_value with packed f16 atomics.  D must be a
 * power of two <= 64 (>= 2 for f16).  im2col_step: the reference's contract (batch % min(batch, step) == 0).
 * ------------------------------------------------------------------------------------------ */
int codetr_msda_backward_f16(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                             const int64_t *level_start_dev, const void *sampling_loc_dev, const void *attn_weight_dev,
                             const void *grad_output_dev, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P,
                             int64_t im2col_step, void *grad_value_dev, void *grad_sampling_loc_dev,
                             void *grad_attn_weight_dev);
int codetr_msda_backward_f32(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                             const int64_t *level_start_dev, const void *sampling_loc_dev, const void *attn_weight_dev,
                             const void *grad_output_dev, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P,
                             int64_t im2col_step, void *grad_value_dev, void *grad_sampling_loc_dev,
                             void *grad_attn_weight_dev);
int codetr_msda_backward_f64(void *stream, const void *value_dev, const int64_t *spatial_shapes_dev,
                             const int64_t *level_start_dev, const void *sampling_loc_dev, const void *attn_weight_dev,
                             const void *grad_output_dev, int64_t B, int64_t S, int M, int D, int L, int64_t Nq, int P,
                             int64_t im2col_step, void *grad_value_dev, void *grad_sampling_loc_dev,
                             void *grad_attn_weight_dev);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension: y[r,:] = (x[r,:] - mean) * rsqrt(var + eps) * gamma + beta
 *
 * Replaces at::native::layer_norm behind every nn.LayerNorm of the hot path (built through mmcv's
 * build_norm_layer at codetr/swin.py:331,345,627 and codetr/transformer_mmcv.py:647; nn.LayerNorm at
 * codetr/transformer.py:153,452).  x, y [rows, C] dense row-major (y may alias x); gamma, beta [C];
 * fp32 statistics (two-pass), one rounding at the store.  C % 8 == 0, C <= 4096.
 * ------------------------------------------------------------------------------------------ */
int codetr_layernorm_f16(void *stream, const void *x_dev, const void *gamma_dev, const void *beta_dev, void *y_dev,
                         int64_t rows, int64_t C, float eps);
int codetr_layernorm_bf16(void *stream, const void *x_dev, const void *gamma_dev, const void *beta_dev, void *y_dev,
                          int64_t rows, int64_t C, float eps);

/* Swin PatchMerging's gather + LayerNorm in one pass (codetr/transformer_mmcv.py:213-316: nn.Unfold(2, stride 2) on
 * the token map, then LayerNorm(4C)): x_dev [B, H, W, C] f16 token map, y_dev [B, ceil(H/2)*ceil(W/2), 4C] f16 with
 * the 4C axis ordered (ky, kx, c) -- gamma / beta (and the reduction Linear's columns) must be in that order, i.e.
 * permuted from nn.Unfold's (c, ky, kx); zeros beyond an odd H / W.  C % 8 == 0, 4C <= 4096. */
int codetr_patch_merge_layernorm_f16(void *stream, const void *x_dev, const void *gamma_dev, const void *beta_dev,
                                     void *y_dev, int64_t B, int64_t H, int64_t W, int64_t C, float eps);
int codetr_patch_merge_layernorm_bf16(void *stream, const void *x_dev, const void *gamma_dev, const void *beta_dev,
                                     void *y_dev, int64_t B, int64_t H, int64_t W, int64_t C, float eps);  /* bf16 storage, same contract */

/* ------------------------------------------------------------------------------------------
 * Fused (shifted-)window multi-head self-attention of one Swin block.
 *
 * Replaces the tensor program of ShiftWindowMSA.forward + WindowMSA.forward between the qkv and
 * the proj Linear (reference codetr/swin.py:191-252 and :92-112): pad-to-window, roll(-shift),
 * window_partition, q*scale, q@k^T, + relative position bias, + shift mask (-100), softmax,
 * attn@v, head merge, window_reverse, roll(+shift), crop.
 *
 *   qkv_dev      [B, H*W, 3*C]  f16  output of the qkv Linear on the UNPADDED, unrolled token map;
 *                                    channel order (q | k | v), each head-major (C = num_heads*head_dim)
 *   qkv_bias_dev [3*C]          f16  bias of that Linear (what a zero pad token turns into; zeros
 *                                    if the layer has no bias) -- pad tokens take part in the
 *                                    softmax as keys, exactly as in the reference
 *   rel_bias_dev [num_heads, N, N] f16  gathered relative position bias, N = window_size^2
 *   out_dev      [B, H*W, C]    f16  attention output in the same spatial token order
 *   shift        0 (W-MSA) or window_size/2 (SW-MSA); head_dim must be 32; window_size in {4,7,8,12}
 *
 * fp32 scores / softmax / accumulation; probabilities rounded to f16 (bf16 in the _bf16 form, all tensors bf16) for
 * the P.V product.
 * ------------------------------------------------------------------------------------------ */
int codetr_window_attention_f16(void *stream, const void *qkv_dev, const void *qkv_bias_dev,
                                const void *rel_bias_dev, void *out_dev, int64_t B, int64_t H, int64_t W,
                                int num_heads, int head_dim, int window_size, int shift);
int codetr_window_attention_bf16(void *stream, const void *qkv_dev, const void *qkv_bias_dev,
                                 const void *rel_bias_dev, void *out_dev, int64_t B, int64_t H, int64_t W,
                                 int num_heads, int head_dim, int window_size, int shift);
/* The same attention with the output emitted as OCP e4m3 bytes, out8[i] = sat(f16(o[i]) / out_scale): the operand of
 * the fp8 proj GEMM (BASELINE config 5) without the 16-bit tensor's round trip: codetr_cast_fp8_f16 applied to the
 * kernel's own fp16 result (tests: equal to the two-kernel path but for ~1 element per million on a rounding boundary).  out8_dev [B, H*W, C] bytes, 4-byte aligned. */
int codetr_window_attention_fp8out_f16(void *stream, const void *qkv_dev, const void *qkv_bias_dev,
                                       const void *rel_bias_dev, void *out8_dev, float out_scale, int64_t B,
                                       int64_t H, int64_t W, int num_heads, int head_dim, int window_size, int shift);
/* Round 6: every form above through ONE entry, plus the layout of the relative-position bias.
 *   elem        0: fp16 tensors, 1: bf16 (out_mode 0 only)
 *   out_mode    0: 16-bit output (codetr_window_attention_f16 / _bf16); 1: e4m3 = sat(f16(o) / out_scale)
 *               (codetr_window_attention_fp8out_f16); 2: e4m3 + MX block scales in out_scales_dev
 *               (codetr_window_attention_fp8mx_f16).  out_scales_dev / out_scale are ignored by the modes that do not use them.
 *   bias_layout 0: rel_bias_dev is the reference's gathered table [nH, N, N] (swin.py:92-112: table[index].view(N, N, nH)
 *               permuted), as above; 1: the same values in the LANE ORDER of the kernel's score tiles -- row q of head h
 *               holds at position j the bias of key idx[j], idx from codetr_window_attention_bias_index (window sizes 12,
 *               8, 4: whole 16-key tiles).  A lane's values of a query tile are then contiguous (72 bytes for the 12 x 12
 *               window: five loads instead of nine 8-byte pieces 32 bytes apart), results are bit-identical to layout 0,
 *               launches 4-12 % shorter (profiles/r06_window_attention.txt).  The table is a per-layer constant: the host
 *               permutes it once (codetr/swin.py: WindowMSA.relative_position_bias).
 * codetr_window_attention_bias_index: idx_host[window_size^2]; CODETR_E_UNSUPPORTED for window sizes without the lane order. */
int codetr_window_attention_ex(void *stream, const void *qkv_dev, const void *qkv_bias_dev, const void *rel_bias_dev,
                               void *out_dev, void *out_scales_dev, float out_scale, int64_t B, int64_t H, int64_t W,
                               int num_heads, int head_dim, int window_size, int shift, int elem, int out_mode,
                               int bias_layout);
int codetr_window_attention_bias_index(int window_size, int32_t *idx_host);

/* ------------------------------------------------------------------------------------------
 * Dense multi-head softmax attention, head_dim 32: the core of nn.MultiheadAttention(256, 8) in the decoder's
 * self-attention (reference codetr/transformer_mmcv.py:394-428, called from DetrTransformerDecoderLayer,
 * codetr/transformer.py:233-277) between its in- and out-projections, which are codetr_linear_* calls:
 *   out[b, i, h*32 + c] = sum_j softmax_j(q[b,i,h,:] . k[b,j,h,:] / sqrt(32)) * v[b, j, h*32 + c]
 *   q_dev   [B, Nq, >= H*32]  rows q_row_stride elements apart (q and k may be column ranges of one fused projection)
 *   k_dev, v_dev [B, Nk, ...] likewise;  out_dev [B, Nq, ...] rows out_row_stride apart
 * No attention / key-padding mask (the inference path has none).  fp32 scores, online softmax over 128-key chunks,
 * fp32 accumulation.  Nk <= 1024 (K and V of one head live in LDS), head_dim == 32: CODETR_E_UNSUPPORTED otherwise.
 * ------------------------------------------------------------------------------------------ */
int codetr_mha_attention_f16(void *stream, const void *q_dev, const void *k_dev, const void *v_dev, void *out_dev,
                             int64_t B, int64_t Nq, int64_t Nk, int num_heads, int head_dim, int64_t q_row_stride,
                             int64_t k_row_stride, int64_t v_row_stride, int64_t out_row_stride);
int codetr_mha_attention_bf16(void *stream, const void *q_dev, const void *k_dev, const void *v_dev, void *out_dev,
                              int64_t B, int64_t Nq, int64_t Nk, int num_heads, int head_dim, int64_t q_row_stride,
                              int64_t k_row_stride, int64_t v_row_stride, int64_t out_row_stride);

/* ------------------------------------------------------------------------------------------
 * One DINO decoder layer's row-local work in one launch (csrc/decoder_layer.hip), f16, embed_dims 256, 8 heads of 32,
 * 4-d reference boxes, post-norm layer (self_attn, norm, cross_attn, norm, ffn, norm) with box refinement.
 * Replaces, per layer, the ~19 launches of reference codetr/transformer.py:193-230 (DinoTransformerDecoder.forward:
 * reference-point scaling, gen_sineembed_for_position :157-190, ref_point_head, the layer, reg_branches[lid]) and
 * :233-277 / transformer_mmcv.py:583-749 (the layer's operation_order) -- everything except softmax(QK^T)V of the
 * self-attention, which stays codetr_mha_attention_f16 between two of these launches:
 *   TAIL (attn_dev != NULL): x1 = LN1(x + attn.Wo^T + bo); (offsets | logits) = (x1 + qpos).Wol^T + bol;
 *        s = MSDA(value, softmax(logits), ref_xy + off / P * ref_wh / 2) with ref = sigmoid(ref_dev) * valid ratios (fp32);
 *        x2 = LN2(x1 + s.Wout^T + bout); x3 = LN3(x2 + relu(x2.W1^T + b1).W2^T + b2); ref_out = ref + reg_branch(x3)
 *   HEAD (head_w_dev != NULL): qpos_out = ref_point_head(sine_embed(sigmoid(ref') * valid_ratios[level 0]));
 *        qk_out = (x3 + qpos_out).Wqk^T + bqk; v_out = x3.Wv^T + bv       (ref' = ref_out, or ref_dev without a TAIL;
 *        x3 = x_dev without a TAIL)
 *   x_out = x3 with a HEAD, else final_norm(x3) (the decoder's output LayerNorm, final_norm_dev = gamma | beta).
 * Tensors: x, attn, qpos, x_out, qpos_out, v_out [B*Nq, 256]; qk_out [B*Nq, 512]; ref, ref_out [B*Nq, 4] unactivated;
 * valid_ratios32 [B, L, 2] fp32; value [B, S, 8, 32] (the layer's projected, masked value map); spatial_shapes [L, 2],
 * level_start [L] int64 on the device.  Packed f16 weights: matrices first, FRAGMENT-MAJOR -- a [N][K] nn.Linear weight
 * is stored as N/16 x K/32 blocks of 64 x 8 halfs, block (tile, ks) at ((tile * K/32 + ks) * 64 + lane) * 8 with
 * lane = 16 g + r holding W[16 tile + r][32 ks + 8 g .. + 7] (one wave load = 1 KB of whole lines, the MFMA operand
 * layout) -- then the small vectors, which the kernel copies to LDS once; in this order:
 *   tail_w: Wo, Wol (offsets rows then logits rows: 8*L*P*2 + 8*L*P, zero rows up to 512), Wout, W1 [2048][256],
 *           W2 [256][2048], Wr1, Wr2, Wr3 (4 rows + 12 zero rows) | bo, LN1 gamma, beta, bol, bout, LN2 gamma, beta, b1,
 *           b2, LN3 gamma, beta, br1, br2, br3 (4 values + 4 of padding)
 *   head_w: Wqk [512][256], Wv [256][256] | bqk, bv       pos_w: Wp1 [256][512], Wp2 | bp1, bp2      final_norm: gamma, beta
 * codetr_decoder_layer_blob_halfs(which = 0 tail | 1 head | 2 pos | 3 final norm, ...) returns the element counts.
 * Rounding points are those of the separate kernels (f16 wherever they materialise a tensor; fp32 statistics, softmax,
 * sampling arithmetic and accumulation); the results differ from them only by summation order.
 * CODETR_E_UNSUPPORTED outside L*P <= 32, hidden == 2048, (8*L*P*3) % 16 == 0 and <= 512.
 * ------------------------------------------------------------------------------------------ */
int codetr_decoder_layer_supported(int embed_dims, int num_heads, int num_levels, int num_points, int hidden, int ref_dim,
                                   int pos_feat);
int64_t codetr_decoder_layer_blob_halfs(int which, int num_levels, int num_points, int hidden);
int codetr_decoder_layer_f16(void *stream, const void *x_dev, const void *attn_dev, const void *qpos_dev,
                             const void *ref_dev, const float *valid_ratios32_dev, const void *value_dev,
                             const int64_t *spatial_shapes_dev, const int64_t *level_start_dev, const void *tail_w_dev,
                             const void *pos_w_dev, const void *head_w_dev, const void *final_norm_dev, void *x_out_dev,
                             void *ref_out_dev, void *qpos_out_dev, void *qk_out_dev, void *v_out_dev, int64_t B,
                             int64_t Nq, int64_t S, int num_levels, int num_points, int hidden, float ln_eps,
                             float temperature);
/* bf16 twin: bf16 activations / weights / outputs, v_mfma_f32_16x16x32_bf16, the same fp32 arithmetic in between (the
 * kernel template of csrc/decoder_layer.hip instantiated on the bf16 element trait). */
int codetr_decoder_layer_bf16(void *stream, const void *x_dev, const void *attn_dev, const void *qpos_dev,
                             const void *ref_dev, const float *valid_ratios32_dev, const void *value_dev,
                             const int64_t *spatial_shapes_dev, const int64_t *level_start_dev, const void *tail_w_dev,
                             const void *pos_w_dev, const void *head_w_dev, const void *final_norm_dev, void *x_out_dev,
                             void *ref_out_dev, void *qpos_out_dev, void *qk_out_dev, void *v_out_dev, int64_t B,
                             int64_t Nq, int64_t S, int num_levels, int num_points, int hidden, float ln_eps,
                             float temperature);

/* ------------------------------------------------------------------------------------------
 * GroupNorm on token-major activations, written into a slice of the flattened multi-level map.
 *
 * Replaces nn.GroupNorm(32, 256) of the ChannelMapper neck (mmdet v3.3.0, built at
 * codetr/codetr.py:53-54 from configs lsj:40-47) together with the flatten / transpose / cat copies
 * that turn the NCHW levels into the encoder's [B, S, C] input (codetr/transformer.py:508-519).
 *
 *   x_dev   [B, HW, C] f16 (output of the level's 1x1 conv run as a linear over tokens)
 *   out_dev points at row `level_start` of image 0 in the [B, S, C] destination;
 *           out_batch_stride = S*C elements between images
 *   workspace_dev: codetr_groupnorm_tokens_workspace_bytes(B, HW, C) bytes of device scratch
 *   groups must equal C/8 (8 channels = one 16-byte chunk per group: GN(32) on 256 channels)
 * Statistics over (HW x 8) per (image, group): fp32 partial sums of x and x^2 per 128-row slab, fp64 final reduction.
 * fp32 partials lose about 1e-7 mean^2 / var of rstd, so the final reduction bounds that loss from the sums themselves
 * and, where it may exceed 2^-13 (f16) / 2^-10 (bf16) of var + eps (mean^2 / var above about 4 / 39 at C = 256), the
 * group's sums are taken again over the same grid about the pivot K = (float)mean of the first reduction:
 * mean = K + s/n, var = q/n - (s/n)^2.  A call with such groups costs up to one more pass over x; a call without them two
 * launches that return at once.  That the neck's activations stay below the threshold is measured with seeded random
 * weights only, not with a trained checkpoint.
 * ------------------------------------------------------------------------------------------ */
int64_t codetr_groupnorm_tokens_workspace_bytes(int64_t B, int64_t HW, int64_t C);
int codetr_groupnorm_tokens_f16(void *stream, const void *x_dev, const void *gamma_dev, const void *beta_dev,
                                void *out_dev, int64_t out_batch_stride, void *workspace_dev, int64_t B, int64_t HW,
                                int64_t C, int groups, float eps);
int codetr_groupnorm_tokens_bf16(void *stream, const void *x_dev, const void *gamma_dev, const void *beta_dev,
                                void *out_dev, int64_t out_batch_stride, void *workspace_dev, int64_t B, int64_t HW,
                                int64_t C, int groups, float eps);  /* bf16 storage, same contract */

/* ------------------------------------------------------------------------------------------
 * Sine positional encoding of one pyramid level, written into a slice of lvl_pos_embed [B, S, 2*num_feats].
 *
 * Replaces SinePositionalEncoding.forward (codetr/positional_encoding.py:58-93) and the flatten / transpose /
 * "+ level_embeds[lvl]" / cat steps of CoDinoTransformer.forward (codetr/transformer.py:508-519).
 *   ycum_dev, xcum_dev [B, H, W] f32: running sums of (1 - mask) along y and along x (host: two cumsum calls)
 *   level_embed_dev    [2*num_feats] f16 or NULL
 *   out_dev            row `level_start` of image 0 in the [B, S, 2*num_feats] destination; out_batch_stride =
 *                      S * 2*num_feats elements between images
 * channel layout [pos_y | pos_x], inside each: channel 2f = sin(e / T^(2f/num_feats)), 2f+1 = cos(same),
 * e = (cum + offset) / (last + eps) * scale when `normalize`, else cum.  fp32 arithmetic, f16 result.
 * ------------------------------------------------------------------------------------------ */
int codetr_sine_pos_tokens_f16(void *stream, const float *ycum_dev, const float *xcum_dev, const void *level_embed_dev,
                               void *out_dev, int64_t out_batch_stride, int64_t B, int64_t H, int64_t W, int num_feats,
                               float temperature, float scale, float eps, float offset, int normalize);
int codetr_sine_pos_tokens_bf16(void *stream, const float *ycum_dev, const float *xcum_dev, const void *level_embed_dev,
                               void *out_dev, int64_t out_batch_stride, int64_t B, int64_t H, int64_t W, int num_feats,
                               float temperature, float scale, float eps, float offset, int normalize);  /* bf16 storage, same contract */

/* ------------------------------------------------------------------------------------------
 * Fused transformer FFN:  y = x + relu(x . w1^T + b1) . w2^T + b2      (hidden activation never leaves the CU)
 *
 * Replaces FFN.forward (codetr/transformer_mmcv.py:484-500: Linear, ReLU, Linear, + identity) of the deformable
 * encoder / DINO decoder layers (configs lsj:72-79, 92-99: embed_dims 256, feedforward_channels 2048).
 *   x_dev [M, 256]; w1_dev [hidden, 256]; b1_dev [hidden]; b2_dev [256]; y_dev [M, 256]; all f16
 *   w2_packed_dev [256, hidden]: the second Linear's weight passed ONCE through codetr_ffn_pack_w2_f16 (a column
 *   permutation inside every 64-block that puts the hidden units in the order the first product's accumulators
 *   hold them, so that those accumulators feed the second product without leaving registers)
 * C_in must be 256, hidden a multiple of 64; all device pointers 16-byte aligned (CODETR_E_BADARG otherwise).  fp32
 * accumulation; the hidden activation is rounded to f16 between the two products and the FFN output once more before
 * the residual add (as the two-kernel f16 path does).
 * ------------------------------------------------------------------------------------------ */
int codetr_ffn_relu_f16(void *stream, const void *x_dev, const void *w1_dev, const void *b1_dev,
                        const void *w2_packed_dev, const void *b2_dev, void *y_dev, int64_t M, int64_t C_in,
                        int64_t hidden);

/* The same kernel with the layer's next two steps folded into its epilogue (post-norm encoder layer,
 * operation_order (..., 'ffn', 'norm'), codetr/transformer_mmcv.py:649-749, and the `query + query_pos` at the head
 * of the next layer's attention, codetr/multi_scale_deformable_attention.py:161-162):
 *   y      = LayerNorm(x + ffn(x)) * gamma + beta        ln_gamma_dev / ln_beta_dev [256] f16, both or neither
 *   y_plus_pos = y + pos                                  pos_dev / y_plus_pos_dev [M, 256] f16, both or neither
 * The LayerNorm arithmetic is that of codetr_layernorm_f16 (fp32 two-pass statistics over the f16-rounded sum), summed
 * in the accumulators' lane order: equal to running the three kernels one after another up to the last f16 bit of a
 * few outputs (< 2 %); y_plus_pos is exactly y + pos. */
int codetr_ffn_relu_ln_f16(void *stream, const void *x_dev, const void *w1_dev, const void *b1_dev,
                           const void *w2_packed_dev, const void *b2_dev, void *y_dev, int64_t M, int64_t C_in,
                           int64_t hidden, const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps,
                           const void *pos_dev, void *y_plus_pos_dev);

/* ... and with the layer's PRECEDING LayerNorm folded in as well (operation_order (..., 'norm', 'ffn', 'norm')): the
 * kernel normalises its input rows in registers (fp32 two-pass statistics, f16 result = the MFMA operand and the
 * identity), so that norm's output is never written:
 *   x1 = LayerNorm(x) * ln_in_gamma + ln_in_beta;  y = LayerNorm(x1 + ffn(x1)) * gamma + beta;  y_plus_pos = y + pos
 * ln_in_gamma_dev / ln_in_beta_dev [256] f16, both or neither (NULL: codetr_ffn_relu_ln_f16). */
int codetr_ffn_relu_ln2_f16(void *stream, const void *x_dev, const void *w1_dev, const void *b1_dev,
                            const void *w2_packed_dev, const void *b2_dev, void *y_dev, int64_t M, int64_t C_in,
                            int64_t hidden, const void *ln_in_gamma_dev, const void *ln_in_beta_dev, float ln_in_eps,
                            const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps, const void *pos_dev,
                            void *y_plus_pos_dev);
/* The fused FFN on the e4m3 matrix path (BASELINE config 5; no reference counterpart for 8-bit arithmetic -- the layer
 * is the same FFN, codetr/transformer_mmcv.py:484-500, inside the same post-norm encoder layer :709-749):
 *   x1 = LayerNorm_in(x) (or x);  xq = sat(x1 / x_scale) -> e4m3
 *   h  = relu((xq . w1q^T) * w1_scale[j] * x_scale + b1[j]);  hq = sat(h / h_scale) -> e4m3
 *   y  = LayerNorm(x1 + (hq . w2q^T) * w2_scale[n] * h_scale + b2[n]) * gamma + beta;  y_plus_pos = y + pos
 * x / y / pos / biases / LayerNorm parameters f16 as in codetr_ffn_relu_ln2_f16; w1q_dev [hidden, 256] e4m3 bytes with
 * per-hidden-unit scales w1_scale_dev [hidden] fp32; w2q_packed_dev [256, hidden] e4m3 bytes with per-output-channel
 * scales w2_scale_dev [256] fp32, its columns permuted inside every 128-block: packed column 32 g + 4 t + r holds
 * hidden unit 16 t + 4 g + r of the block (g < 4, t < 8, r < 4 -- the order in which the first product's accumulators
 * become the second product's operand).  x_scale / h_scale: static per-tensor activation scales from calibration.
 * fp32 accumulation with v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales); conversions saturate at +-448.
 * C_in must be 256, hidden a multiple of 128 and <= 2048 (CODETR_E_UNSUPPORTED otherwise); x, y, pos, the weights and
 * the LayerNorm parameters 16-byte aligned (CODETR_E_BADARG). */
int codetr_ffn_fp8(void *stream, const void *x_f16_dev, const void *w1q_dev, const float *w1_scale_dev,
                   const void *b1_f16_dev, const void *w2q_packed_dev, const float *w2_scale_dev,
                   const void *b2_f16_dev, void *y_f16_dev, int64_t M, int64_t C_in, int64_t hidden, float x_scale,
                   float h_scale, const void *ln_in_gamma_dev, const void *ln_in_beta_dev, float ln_in_eps,
                   const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps, const void *pos_dev,
                   void *y_plus_pos_dev);

/* bf16 storage form of the same kernel (all tensors bf16; the packed W2 comes from codetr_ffn_pack_w2_f16, which only
 * moves 16-bit elements) */
int codetr_ffn_relu_ln2_bf16(void *stream, const void *x_dev, const void *w1_dev, const void *b1_dev,
                            const void *w2_packed_dev, const void *b2_dev, void *y_dev, int64_t M, int64_t C_in,
                            int64_t hidden, const void *ln_in_gamma_dev, const void *ln_in_beta_dev, float ln_in_eps,
                            const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps, const void *pos_dev,
                            void *y_plus_pos_dev);
/* one-time weight pre-pack for the call above: w2_dev [C_out, hidden] f16 -> w2_packed_dev (same shape) */
int codetr_ffn_pack_w2_f16(void *stream, const void *w2_dev, void *w2_packed_dev, int64_t C_out, int64_t hidden);
/* The post-norm encoder layer from the attention output to the layer output as ONE launch (reference
 * codetr/transformer_mmcv.py: BaseTransformerLayer.forward, operation_order self_attn - norm - ffn - norm, with the tail of
 * MultiScaleDeformableAttention.forward, multi_scale_deformable_attention.py: `output_proj(output) + identity`):
 *     x0 = identity + E(attn @ Wo^T + bo)       (E: rounded to the storage type, as the separate GEMM's epilogue does)
 *     x1 = LayerNorm_in(x0)                      (ln_in_* NULL: x1 = x0)
 *     y  = LayerNorm(x1 + relu(x1 @ W1^T + b1) @ W2^T + b2),   y_plus_pos = y + pos (optional, as above)
 * attn_dev / identity_dev / y_dev [M, 256]; wo_dev [256, 256], bo_dev [256]: nn.Linear parameters as they are;
 * w1_perm_dev [hidden, 256]: W1 with its COLUMNS reordered by codetr_ffn_oproj_w1_index (column j <- column idx[j]; the
 * kernel produces x1 in its epilogue's lane layout and multiplies it as it is); w2_packed_dev from
 * codetr_ffn_pack_w2_f16.  Replaces a GEMM launch that reads attn and identity and writes x0, and the FFN kernel's read of
 * x0: 1.7 GB -> 0.84 GB of HBM traffic per layer at four 1920x1280 images, for 6 % more MFMA work.  Same argument checks
 * as codetr_ffn_relu_ln2_f16. */
int codetr_ffn_oproj_relu_ln2_f16(void *stream, const void *attn_dev, const void *wo_dev, const void *bo_dev,
                                  const void *identity_dev, const void *w1_perm_dev, const void *b1_dev,
                                  const void *w2_packed_dev, const void *b2_dev, void *y_dev, int64_t M, int64_t C_in,
                                  int64_t hidden, const void *ln_in_gamma_dev, const void *ln_in_beta_dev,
                                  float ln_in_eps, const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps,
                                  const void *pos_dev, void *y_plus_pos_dev);
int codetr_ffn_oproj_relu_ln2_bf16(void *stream, const void *attn_dev, const void *wo_dev, const void *bo_dev,
                                   const void *identity_dev, const void *w1_perm_dev, const void *b1_dev,
                                   const void *w2_packed_dev, const void *b2_dev, void *y_dev, int64_t M, int64_t C_in,
                                   int64_t hidden, const void *ln_in_gamma_dev, const void *ln_in_beta_dev,
                                   float ln_in_eps, const void *ln_gamma_dev, const void *ln_beta_dev, float ln_eps,
                                   const void *pos_dev, void *y_plus_pos_dev);
/* idx_host[C_in] (C_in = 256): source column of W1 for every column of w1_perm_dev.  Host-only. */
int codetr_ffn_oproj_w1_index(int64_t C_in, int32_t *idx_host);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_HIP_H_ */
