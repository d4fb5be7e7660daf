/* codetr_raw.h -- companion header of codetr_hip.h: raw Bayer sensor frames -- one sample per pixel, 8 to 16 bits, as
 * GenICam's BayerXX8/10/12/16 and V4L2's SRGGB8/10/12 deliver them -- demosaiced into the packed RGB uint8 images every
 * kernel of the Inferencer reads.  Exported from the same libcodetr_hip.so, versioned on its own.  Error codes and the
 * limits CODETR_PREPROCESS_BATCH_MAX / CODETR_FRAME_MAX_SIDE are codetr_hip.h's.
 *
 * The rule, in exact integers.  A frame is H x W samples s[y][x], H, W >= 1, uint8 (bits = 8) or the little-endian uint16
 * container with the sample in its low `bits` bits (bits = 9..16).  The pattern names the colours of the sites (0,0), (0,1),
 * (1,0), (1,1) and repeats with period 2 on both axes; its code is the position of the red site, 2 ry + rx: the site
 * (y, x) is red when (y & 1, x & 1) = (ry, rx), blue when both differ, green otherwise.
 *  1. Normalise.  c = the colour of the site; m_c = floor(gain_c * 4294901760.0 / (white - black) + 0.5) in IEEE double
 *     (4294901760 = 65535 * 65536), computed once on the host (codetr_raw_multipliers), 0 <= m_c < 2^32, white > black.
 *       v = min(65535, (max(min(s, white) - black, 0) * m_c + 2^15) >> 16)          product and sum in 64 bits
 *     (x <= 65535 and m_c < 2^32: the sum is below 2^48.)  White balance acts on the mosaic, before interpolation.
 *  2. Borders: whole-sample reflection that does not repeat the edge.  An index i on an axis of length n reads
 *     fold(i, n): n = 1 -> 0; else m = i mod (2 n - 2), non-negative, and m < n ? m : 2 n - 2 - m.  The period is even, so
 *     fold keeps the parity of i and with it the site's colour: no border site needs a filter of its own.  What is read
 *     is v of step 1, normalised as the colour of the sample's OWN site -- which matters on an axis of length 1 only,
 *     where a neighbour of the other parity reads sample 0.
 *  3. Demosaic.  With C = v at the site, and the sums over the folded neighbours
 *       H1 = v[y][x-1] + v[y][x+1]   V1 = v[y-1][x] + v[y+1][x]   H2 = v[y][x-2] + v[y][x+2]   V2 = v[y-2][x] + v[y+2][x]
 *       D = v[y-1][x-1] + v[y-1][x+1] + v[y+1][x-1] + v[y+1][x+1]
 *     method CODETR_RAW_MALVAR (Malvar, He, Cutler 2004, every coefficient doubled: integers over 16, each filter sums
 *     to 16):
 *       green at a red / blue site                         S = 8 C + 4 (H1 + V1) - 2 (H2 + V2)
 *       red (blue) at a green site in a red (blue) row     S = 10 C + 8 H1 - 2 H2 + V2 - 2 D
 *       red (blue) at a green site in a blue (red) row     S = 10 C + 8 V1 - 2 V2 + H2 - 2 D
 *       red at a blue site, blue at a red site             S = 12 C + 4 D - 3 (H2 + V2)
 *       d = min(65535, max(0, (S + 8) >> 4))               >> arithmetic, S in int32
 *     Width: every v is in [0, 65535]; the positive coefficients of a filter sum to at most 28 and the negative ones to
 *     at least -12, so -786420 <= S <= 1834980 < 2^31.
 *     method CODETR_RAW_BILINEAR, the 3 x 3 averages:
 *       green at a red / blue site (H1 + V1 + 2) >> 2;  the other colour there (D + 2) >> 2;
 *       at a green site the colour of its row (H1 + 1) >> 1, the other one (V1 + 1) >> 1.
 *     Either way the site's own colour is d = C.
 *  4. Tone.  out = lut[d >> 4], a table of 4096 bytes the caller builds (hip_ops.raw_settings: "linear" is
 *     (i * 255 + 2047) / 4095 in integers; "srgb", a gamma or a caller's table otherwise).
 *  5. Output: packed RGB, rows of 3 W bytes, at dst_offset.  No byte outside an image's H * W * 3 is written.
 *
 * How far the rule is from the same computation in real numbers -- vf = min(65535, max(min(s, white) - black, 0) * gain_c
 * * 65535 / (white - black)), df = the filter on vf over 16 clamped to [0, 65535], out_f = 255 df / 65535 for the linear
 * table -- in units of the output byte.  tests/test_raw_cpu.py asserts this bound:
 *   a. |v - vf| <= 1: m_c is within 0.5 of its real value and x = min(s, white) - black <= 65535, so x m_c / 65536 is
 *      within 0.5 * 65535 / 65536 of x M / 65536 (the margin of 2^-17 covers M's evaluation in double), and the rounding
 *      shift adds at most 0.5; min(65535, .) does not widen it.
 *   b. |d - df| <= E: the filter carries (sum |coefficient|) / 16 of (a) -- 32/16, 40/16, 40/16 for the three Malvar
 *      filters, 1 for an average -- and its own rounding shift adds 0.5: E = 3.0 for malvar, 1.5 for bilinear (1 for the
 *      site's own colour); the clamp does not widen it.
 *   c. i = d >> 4 drops r = d - 16 i in 0..15, and 65535 = 16 * 4095 + 15:  d / 65535 - i / 4095 = (4095 r - 15 i) /
 *      (65535 * 4095), of magnitude at most 15 / 65535.
 *   d. the table's entry is within 0.5 of 255 i / 4095.
 *   |out - out_f| <= 0.5 + 255 (15 + E) / 65535: 0.57004 for malvar, 0.56421 for bilinear.  For another tone curve T the
 *   factor 255 / 65535 becomes T's largest slope per unit of d.
 *   Default settings with bits = 8 give m = 257 * 65536, v = 257 s and lut[(257 s) >> 4] = s: a site's own colour leaves
 *   as the input byte.  With bits = 10 or 12 it is round(255 s / white) exactly, with 14 or 16 within 1 of it.
 *
 * codetr_raw_multipliers: HOST only, no HIP call.  gains_host[3] (red, green, blue; finite, >= 0) -> m_host[3] of step 1.
 *   CODETR_E_BADARG for a null pointer, black < 0, white > 65535, white <= black, a gain that is negative or not finite,
 *   or an m_c >= 2^32.
 *
 * codetr_raw_to_rgb_u8: N <= CODETR_PREPROCESS_BATCH_MAX frames in one launch (the caller splits).
 *   src_dev / src_bytes: one device buffer that holds every frame, only read, and never outside [0, src_bytes).
 *   rows_host: HOST [N][CODETR_RAW_ROW_INTS] int64: pattern code, bits, H, W, offset of sample (0, 0) in src_dev, row pitch
 *     in bytes (>= W for bits = 8, >= 2 W above), offset of the image in dst_dev.  The rows of one call share a container:
 *     all bits = 8 or all in 9..16.  A 16-bit frame needs an even address (src_dev + offset) and an even pitch; an 8-bit
 *     frame may have any.
 *   settings_host: HOST [CODETR_RAW_SETTING_INTS] int64: method, black, white, m_red, m_green, m_blue.
 *   lut_dev: the 4096 bytes of step 4 on the device, 16-byte aligned, only read.
 *   dst_dev / dst_bytes: image n is the packed H x W x 3 at its offset.  src and dst are different buffers.
 *   One launch whatever the rows hold (csrc/raw.hip), no allocation, no synchronisation.  All checks run before any HIP
 *   call (csrc/raw_args.h): CODETR_E_BADARG for a null pointer, N <= 0, a buffer size <= 0, an unknown pattern or method,
 *     bits outside 8..16 or of two containers, a side <= 0, a negative offset, a pitch below the row's bytes, an odd address
 *     or pitch of a 16-bit frame, a row outside src_bytes, an image outside dst_bytes, two images that share a byte, src
 *     and dst (or lut and dst) ranges that share a byte, a lut_dev that is not 16-byte aligned, black < 0, white <= black,
 *     white above the largest sample of a row's bits, a multiplier outside [0, 2^32); CODETR_E_TOO_LARGE for N >
 *     CODETR_PREPROCESS_BATCH_MAX or a side above CODETR_FRAME_MAX_SIDE.
 */
#ifndef CODETR_RAW_H_
#define CODETR_RAW_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_RAW_ABI_VERSION 1
#define CODETR_RAW_ROW_INTS 7
#define CODETR_RAW_SETTING_INTS 6
#define CODETR_RAW_LUT_BYTES 4096

#define CODETR_RAW_RGGB 0
#define CODETR_RAW_GRBG 1
#define CODETR_RAW_GBRG 2
#define CODETR_RAW_BGGR 3

#define CODETR_RAW_MALVAR 0
#define CODETR_RAW_BILINEAR 1

int codetr_raw_abi_version(void);
int codetr_raw_multipliers(int64_t black, int64_t white, const double *gains_host, int64_t *m_host);
int codetr_raw_to_rgb_u8(void *stream, const void *src_dev, int64_t src_bytes, int64_t N, const int64_t *rows_host,
                         const int64_t *settings_host, const void *lut_dev, void *dst_dev, int64_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_RAW_H_ */
