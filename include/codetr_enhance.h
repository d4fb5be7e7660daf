/* codetr_enhance.h -- companion header of codetr_hip.h: local contrast enhancement (CLAHE, contrast-limited adaptive
 * histogram equalisation) of the packed RGB uint8 images every kernel of the Inferencer reads.  The luma of a frame is
 * equalised per tile of a gy x gx grid, the tiles' tables are blended bilinearly between tile centres, and the change of
 * luma is added to R, G and B.  Exported from the same libcodetr_hip.so, versioned on its own.  Error codes and the limits
 * CODETR_PREPROCESS_BATCH_MAX / CODETR_FRAME_MAX_SIDE are codetr_hip.h's.
 *
 * Beyond the reference (its callers run cv2.createCLAHE(...).apply(...) on the host).  It is OpenCV's CLAHE on the Y
 * channel of full-range YCbCr with the float steps replaced by exact rounding; parity with cv2 is unpinned (cv2 is not
 * part of this build, and its table and blend round in fp32).
 *
 * The rule is exact, integers only (>> and // are floor operations), so that a restatement (tests/enhance_ref.py)
 * reproduces every byte.  For an H x W image and a grid gy x gx, 1 <= gy <= H, 1 <= gx <= W, both <=
 * CODETR_ENHANCE_MAX_GRID:
 *  1 Tile size.  th = ceil(H / gy), tw = ceil(W / gx), T = th tw.  Admitted: T <= CODETR_ENHANCE_MAX_TILE = 2^22.
 *  2 Luma.  Y = (77 R + 150 G + 29 B + 128) >> 8, in 0..255 (the weights sum to 256).
 *  3 Padding.  The padded plane has gy th x gx tw samples; along an axis of n stored samples index i >= n reads
 *    2 (n - 1) - i (reflect-101).  g th - n <= g - 1 <= n - 1 (th < n / g + 1, g <= n), so i <= 2 (n - 1) and the index
 *    read is in 0..n - 1.
 *  4 Histogram.  Tile (j, i), rows j th .. (j + 1) th - 1 and columns i tw .. (i + 1) tw - 1 of the padded plane, has
 *    the 256-bin histogram h of its T samples.
 *  5 Clip and redistribute, with the clip count C, 1 <= C <= T, which the caller passes per image:
 *      C = max(1, (round(256 clip_limit) T) >> 16) for a clip_limit in [1 / 256, 256], round(x) = floor(x + 1/2); C = T
 *      for "no clipping".
 *    E = sum_b max(h[b] - C, 0);  h[b] = min(h[b], C);  h[b] += E >> 8;  r = E & 255;  if r > 0: s = 256 // r and every
 *    bin b with b % s == 0 and b // s < r gains 1.  Clipped once, not again after the redistribution (as OpenCV).
 *    With C = T, E = 0 and nothing moves: plain adaptive equalisation (global equalisation with a 1 x 1 grid).
 *    The last step is the closed form of OpenCV's loop `for (i = 0; i < 256 && r > 0; i += s, --r) ++h[i]` with s =
 *    max(256 // r, 1) = 256 // r (r <= 255): iteration k = 0, 1, ... visits bin k s while k < r, and the other
 *    condition never ends it first, because k <= r - 1 gives k s <= (r - 1) (256 // r) < 256.  So exactly the bins k s,
 *    k < r, gain 1: those with b % s == 0 and b // s < r.  The sum of h stays T: min() removes E, E >> 8 returns
 *    256 (E >> 8), the r bins the rest.  (tests/test_enhance_cpu.py runs the loop for every r.)
 *  6 Table.  cum[b] = h[0] + ... + h[b];  L[b] = (255 cum[b] + (T >> 1)) // T, in 0..255 (cum[255] = T).
 *  7 Blend.  For pixel (y, x) with luma v:  uy = 2 y + 1 - th,  jy = floor(uy / (2 th)) (-1 .. gy - 1),  wy = uy -
 *    2 th jy in [0, 2 th),  j0 = clamp(jy, 0, gy - 1), j1 = clamp(jy + 1, 0, gy - 1); ux, ix, wx, i0, i1 likewise from x,
 *    tw, gx.  S = (2 th - wy) ((2 tw - wx) L[j0,i0][v] + wx L[j0,i1][v]) + wy ((2 tw - wx) L[j1,i0][v] + wx L[j1,i1][v]);
 *    Y' = (S + 2 T) // (4 T).  The weights sum to 4 T, so Y' is in 0..255.
 *  8 Output.  Each channel c becomes clamp(c + (Y' - Y), 0, 255): Y replaced, Cb and Cr kept, is a shift of R, G and B.
 *    No byte outside an image's rows is written and nothing outside a declared stored row is read.
 *
 * Word widths (every intermediate fits an unsigned 32-bit word when T <= 2^22).  h, C, E, cum <= T <= 2^22.  Step 6: 255
 * cum + (T >> 1) < 256 T <= 2^30.  Step 7: wy <= 2 th, wx <= 2 tw, an inner sum <= 2 tw 255, S <= 4 T 255, S + 2 T <=
 * 1022 T <= 1022 * 2^22 < 2^32, and 4 T <= 2^24.  Only step 5's product round(256 clip_limit) T needs 39 bits; it is
 * the caller's (host) arithmetic.
 *
 * The division of step 7 by a multiplier.  d = 4 T, M = floor(2^32 / d), n = S + 2 T < 2^32, q0 = (n M) >> 32.
 * 2^32 / d - 1 < M <= 2^32 / d, so n / d - n / 2^32 < n M / 2^32 <= n / d, and with n / 2^32 < 1: floor(n / d) - 1 <= q0
 * <= floor(n / d).  One correction is exact: q = q0 + 1 where n - q0 d >= d, else q0 (n - q0 d < 2 d <= 2^25: no wrap).
 *
 * Distance from the real-number computation: Lr[b] = 255 cum[b] / T, the real bilinear blend Yr of the four Lr with the
 * weights of step 7 over 4 T, the output clamp(c + Yr - Y).  Step 6 rounds Lr to the nearest integer: with Lr = k + f / T,
 * L = k + [f >= T - (T >> 1)], so |L - Lr| <= 1/2 for even and odd T alike.  S / (4 T) is a convex combination of the four
 * L, so it lies within 1/2 of Yr, and (S + 2 T) // (4 T) rounds it half up: another 1/2.  The luma itself is not rounded
 * again (histograms need integers: Y is the input of both computations) and the clamp of step 8 is 1-Lipschitz.  So
 *   |out - out_real| <= 1 grey level per channel, = CODETR_ENHANCE_BOUND_HALVES / 2: two roundings of at most 1/2 each,
 * not three.  tests/test_enhance_cpu.py asserts this bound against a float64 evaluation.
 *
 * Slices.  The histogram pass cuts a tile into S bands of sr rows, one 1 KB partial histogram each in the workspace:
 *   sr = max(1, CODETR_ENHANCE_SLICE_PIXELS // tw), S = ceil(th / sr); where S > CODETR_ENHANCE_MAX_SLICES: sr = ceil(th /
 *   CODETR_ENHANCE_MAX_SLICES), S = ceil(th / sr).  Image n's partials are the words [256 (base_n + (j gx + i) S + s), + 256),
 *   base_n the sum of gy gx S over the images before it.  codetr_enhance_workspace_bytes returns 1024 times the total.
 *
 * codetr_enhance_rgb_u8: N <= CODETR_PREPROCESS_BATCH_MAX images in two launches (the caller splits).
 *   src_dev / src_bytes: one device buffer that holds every stored frame.
 *   rows_host: HOST [N][CODETR_ENHANCE_ROW_INTS] int64: H, W, offset of the stored frame in src_dev, its row pitch in bytes
 *     (>= 3 W), offset of the enhanced frame in dst_dev, its row pitch (>= 3 W), gy, gx, C.
 *   dst_dev / dst_bytes: either a buffer whose bytes src's do not meet, or src_dev itself with dst_bytes == src_bytes and
 *     every image's destination offset and pitch equal to its source's: in place, which is legal because a pixel's result
 *     depends on itself and the tables only.  Bytes outside the images' 3 W-byte rows are not written.
 *   ws_dev / ws_bytes: device scratch of at least codetr_enhance_workspace_bytes(N, rows_host) bytes, 4-byte aligned; every
 *     word that is read is written first by the same call (no memset, no atomics on it).
 *   Two launches (csrc/enhance.hip), no allocation, no synchronisation.  All checks run before any HIP call
 *   (csrc/enhance_args.h): CODETR_E_BADARG for a null pointer, N <= 0, a buffer size <= 0, a side <= 0, a grid value
 *     outside 1..CODETR_ENHANCE_MAX_GRID or above its side, T above CODETR_ENHANCE_MAX_TILE, C outside 1..T, a negative
 *     offset, a pitch below 3 W, a row outside its buffer, two enhanced images whose spans (first row's first byte to last row's last) share a byte, src and dst that
 *     overlap without being the in-place form, a workspace that is misaligned, too small or meets src or dst;
 *     CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX or a side above CODETR_FRAME_MAX_SIDE.
 * codetr_enhance_workspace_bytes: the same checks of N and of every row's H, W, gy, gx -> the bytes, or the (negative)
 *   error code.
 */
#ifndef CODETR_ENHANCE_H_
#define CODETR_ENHANCE_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_ENHANCE_ABI_VERSION 1
#define CODETR_ENHANCE_ROW_INTS 9
#define CODETR_ENHANCE_MAX_GRID 32
#define CODETR_ENHANCE_MAX_TILE 4194304
#define CODETR_ENHANCE_SLICE_PIXELS 8192
#define CODETR_ENHANCE_MAX_SLICES 32
#define CODETR_ENHANCE_BOUND_HALVES 2

int codetr_enhance_abi_version(void);
int64_t codetr_enhance_workspace_bytes(int64_t N, const int64_t *rows_host);
int codetr_enhance_rgb_u8(void *stream, const void *src_dev, int64_t src_bytes, int64_t N, const int64_t *rows_host,
                          void *dst_dev, int64_t dst_bytes, void *ws_dev, int64_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_ENHANCE_H_ */
