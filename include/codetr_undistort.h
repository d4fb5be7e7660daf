/* codetr_undistort.h -- companion header of codetr_hip.h: lens undistortion of the packed RGB uint8 images every kernel
 * of the Inferencer reads.  A stored frame, taken through a lens that follows OpenCV's rational ("Brown") model or its
 * fisheye (Kannala-Brandt) model, is remapped into the rectilinear image of a chosen camera matrix, bilinear taps at
 * 1/32 pixel, a constant border.  Exported from the same libcodetr_hip.so, versioned on its own.  Error codes and the
 * limits CODETR_PREPROCESS_BATCH_MAX / CODETR_FRAME_MAX_SIDE are codetr_hip.h's.
 *
 * Beyond the reference (its callers hand over rectilinear images).  Limits: no rotation R (stereo rectification), no
 * thin-prism or tilted-sensor terms, no automatic framing, bilinear only; parity with cv2.undistort / cv2.remap is
 * unpinned (cv2 is not part of this build) -- the model formulas and INTER_BITS = 5 are OpenCV's, the arithmetic below is
 * this header's own.
 *
 * The rule is exact: integers, and fp32 with one IEEE rounding per named operation and no fused multiply-add, so that a
 * restatement (tests/undistort_ref.py) reproduces every byte.  a (+) b, a (-) b, a (*) b, a (/) b are the fp32
 * operations, sqrt the correctly rounded fp32 root.  Parameters are fp32: (fx, fy, cx, cy) of the camera that took the
 * frame, (fx', fy', cx', cy') of the rectified image, eight coefficients.  Integer coordinates are pixel centres.
 * For output pixel (u, v), 0 <= u < W', 0 <= v < H':
 *  1 Normalise.  x = (float(u) (-) cx') (/) fx';  y = (float(v) (-) cy') (/) fy'.
 *  2 Distort.  xx = x (*) x;  yy = y (*) y;  r2 = xx (+) yy.
 *    CODETR_UNDISTORT_BROWN, coefficients in OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6 (those not given are 0):
 *      num = 1 (+) r2 (*) (k1 (+) r2 (*) (k2 (+) r2 (*) k3));   den = 1 (+) r2 (*) (k4 (+) r2 (*) (k5 (+) r2 (*) k6));
 *      kr = num (/) den;   xy = x (*) y;
 *      xd = ((x (*) kr) (+) ((p1 (+) p1) (*) xy)) (+) (p2 (*) (r2 (+) (xx (+) xx)));
 *      yd = ((y (*) kr) (+) ((p2 (+) p2) (*) xy)) (+) (p1 (*) (r2 (+) (yy (+) yy))).
 *    CODETR_UNDISTORT_FISHEYE, coefficients k1 k2 k3 k4 (then four zeros):
 *      r = sqrt(r2);   t = ATAN(r);   t2 = t (*) t;
 *      td = t (*) (1 (+) t2 (*) (k1 (+) t2 (*) (k2 (+) t2 (*) (k3 (+) t2 (*) k4))));
 *      s = td (/) r, and s = 1 where r2 == 0;   xd = x (*) s;   yd = y (*) s.
 *    ATAN is this header's own, not a runtime's atanf (whose last bit differs between libraries):
 *      z = r where r <= 1, else z = 1 (/) r;   w = z (*) z;
 *      p = c7;  p = c_k (+) w (*) p  for k = 6, 5, ..., 0;   q = z (*) p;
 *      ATAN(r) = q where r <= 1, else 0x1.921fb6p+0 (-) q                          (pi / 2 rounded to fp32)
 *      c0 = 0x1p+0           c1 = -0x1.5550f2p-2   c2 = 0x1.98d60ep-3    c3 = -0x1.1e3d86p-3
 *      c4 = 0x1.912bdep-4    c5 = -0x1.d947a4p-5   c6 = 0x1.797cd6p-6    c7 = -0x1.1d6f08p-8
 *    The degree (15, eight terms) was chosen so that at CODETR_UNDISTORT_MAX_FOCAL the arc tangent's share of the
 *    sampling position, focal * |ATAN - atan| with zero coefficients, stays under a quarter of step 3's 1/32 pixel:
 *    measured over a dense grid of [0, 1e8] and every fp32 within 4096 ulps of the reduction point 1,
 *    |ATAN(r) - atan(r)| <= 1.91e-7 (the polynomial alone 4.9e-8, the rest is fp32 rounding; seven terms give 4.8e-7 and
 *    miss the criterion, nine give 1.71e-7 and no more).  DELTA = 2^-22 = 2.39e-7 bounds it, tests/test_undistort_cpu.py
 *    asserts that, and 16384 * DELTA = 1/256 pixel, half of the quarter step 1/128.
 *  3 Project and quantise.  us = (fx (*) xd) (+) cx;   vs = (fy (*) yd) (+) cy;
 *    X = floor((us (*) 32) (+) 0.5), Y = floor((vs (*) 32) (+) 0.5) as integers: 5 fractional bits.  If either value is
 *    a NaN or outside [-2^20, 2^20] the pixel is `fill` and steps 4 does not apply.
 *  4 Sample.  xi = X >> 5 (arithmetic), a = X & 31;  yi = Y >> 5, b = Y & 31.  The taps p00, p01, p10, p11 are the
 *    stored pixels (yi, xi), (yi, xi + 1), (yi + 1, xi), (yi + 1, xi + 1); a tap outside [0, H) x [0, W) is `fill`
 *    (a constant border, the only mode).  Per channel
 *      out = ((32 - a) (32 - b) p00 + a (32 - b) p01 + (32 - a) b p10 + a b p11 + 512) >> 10.
 *  5 Output.  No byte outside an image's H' W' 3 is written and nothing outside a declared stored row is read.
 *
 * Admitted ranges (the entry point refuses anything else): every parameter finite; focal lengths in (0,
 * CODETR_UNDISTORT_MAX_FOCAL]; |cx|, |cy|, |cx'|, |cy'| <= CODETR_UNDISTORT_MAX_CENTRE; sides in 1..CODETR_FRAME_MAX_SIDE.
 *
 * Identity.  With zero coefficients, (fx', fy', cx', cy') = (fx, fy, cx, cy) and H', W' = H, W the rule returns the input
 * byte for byte.  Proof, with e = 2^-24 (every operation's relative error) : brown gives num = den = kr = 1, the two
 * tangential terms are 0, so xd = x exactly; fisheye is NOT an identity (it maps r to atan r).  d = float(u) (-) cx, x = d
 * (/) fx, m = fx (*) x each round once, so m differs from u - cx by at most 3 e |u - cx| (1 + e)^2; |u - cx| < 32767 +
 * 32768 < 2^16, so |m - (u - cx)| < 3.0001 * 2^-8 = 0.011720; us = m (+) cx adds at most
 * e * 2^15 = 2^-9 = 0.001954 (|us| < 2^15 + 1).  Together < 0.013674 < 1/64, so us * 32 + 0.5 lies strictly between
 * 32 u and 32 u + 1 (its own rounding, below 2^-4 * 2^-24 * 2^21, cannot reach either end), X = 32 u, a = 0, and likewise
 * Y = 32 v, b = 0: out = (1024 p00 + 512) >> 10 = p00.  The centre limit 32768 is what this proof needs: at 65536 the sum
 * passes 1/64.
 *
 * Bound 1, |X / 32 - us_real| <= 1/64 + E, where us_real is steps 1-3 in real numbers (real atan) on the same fp32
 * parameters and X is valid (step 3).  Below, every symbol is the real-number value at the pixel, e = 2^-24, and the
 * usual first-order model holds: a product or quotient adds the relative errors of its operands plus e, a sum adds their
 * absolute errors plus e times its result; the factor G = 1 + 2^-8 covers the products of errors, under the condition
 * written with each model.
 *   x, y carry 2 e relative (subtract, divide); xx, yy, xy 5 e; r2 6 e (a sum of non-negatives).
 *   brown.  Sn = 1 + r2 (|k1| + r2 (|k2| + r2 |k3|)), Sd the same of k4 k5 k6.  Horner's six operations cost 6 e Sn, the
 *     6 e on r2 moves num by at most 6 e r2 |num'(r2)| <= 18 e Sn: |d num| <= 24 e Sn, |d den| <= 24 e Sd, and
 *       Ek = e (24 Sn / |den| + 24 Sd |kr| / |den| + |kr|) bounds |d kr|      (condition: 24 e Sd <= 2^-10 |den|).
 *     x (*) kr: |x| Ek + 3 e |x kr|;  (2 p1) (*) xy: 6 e |2 p1 x y|;  p2 (*) (r2 (+) 2 xx): 8 e |p2| (r2 + 2 xx);  the two
 *     sums add 2 e of the terms' magnitudes.  With Tx = |x kr| + |2 p1 x y| + |p2| (r2 + 2 xx):
 *       |d xd| <= |x| Ek + 10 e Tx;   fx (*) xd and (+) cx add e |fx xd| + e |us|;   the quantiser adds e (|us| + 1/64):
 *       E_brown = G (fx (|x| Ek + 11 e Tx) + e (2 |us| + 1)).
 *   fisheye.  r carries 4 e (6 e halved by the root, plus e).  |d t| <= Dt = DELTA + 4 e t, because atan's slope is
 *     1 / (1 + r2) and r / (1 + r2) <= atan r.  t2: 2 t Dt + e t2.  With P the polynomial factor of td, Sp the same with
 *     |k|: Horner's eight operations cost 8 e Sp and d t2 moves P by at most 4 (Sp / t2) |d t2|: |d P| <= Sp (12 e + 8 Dt
 *     / t).  td = t (*) P: |d td| <= Etd = |P| Dt + Sp (12 e t + 8 Dt) + e |td|.  s = td (/) r and xd = x (*) s add 8 e
 *     relative and |x| / r <= 1: |d xd| <= Etd + 8 e |xd|  (no condition: the only divisor, r, carries 4 e; at r2 = 0
 *     xd = x exactly).
 *       E_fisheye = G (fx (Etd + 9 e |xd|) + e (2 |us| + 1)).
 *   The same holds for Y, vs with y, fy, cy, p1 and p2 exchanged.  At a 1920-wide image, fx = 1000 and mild coefficients E is
 *   about 0.002 pixel (brown) and 0.004 (fisheye, of which fx DELTA is 0.00024); it grows with fx (|x| + |y|), which is the
 *   admitted coordinate range: at most 2^15 + 2^15 for a valid X.
 * Bound 2, against the real bilinear interpolation B(us_real, vs_real) of the stored image continued by `fill`:
 *   |out - B| <= 1/2 + D (|X / 32 - us_real| + |Y / 32 - vs_real|) <= 1/2 + D (1/32 + Ex + Ey),
 *   D the largest difference between two horizontally or vertically neighbouring pixels of the continued image (B is
 *   continuous and piecewise bilinear, so D is its slope bound along either axis; step 4 is B at (X / 32, Y / 32)
 *   exactly, rounded half up).  tests/test_undistort_cpu.py asserts both bounds against a float64 evaluation.
 *
 * codetr_undistort_rgb_u8: N <= CODETR_PREPROCESS_BATCH_MAX images in one launch (the caller splits).
 *   src_dev / src_bytes: one device buffer that holds every stored frame, only read.
 *   rows_host: HOST [N][CODETR_UNDISTORT_ROW_INTS] int64: model, H, W, offset of the stored frame in src_dev, its row pitch
 *     in bytes (>= 3 W), H', W', offset of the rectified image in dst_dev, fill as 0xRRGGBB.
 *   params_host: HOST [N][CODETR_UNDISTORT_PARAM_FLOATS] float: fx fy cx cy, fx' fy' cx' cy', the eight coefficients in
 *     their model's order (unused ones 0).
 *   dst_dev / dst_bytes: image n is the packed H' x W' x 3 at its offset; bytes outside the images are not written.
 *   One launch (csrc/undistort.hip), no allocation, no synchronisation.  All checks run before any HIP call
 *   (csrc/undistort_args.h): CODETR_E_BADARG for a null pointer, N <= 0, a buffer size <= 0, an unknown model, a side
 *     <= 0, a negative offset, a pitch below 3 W, a stored row outside src_bytes, a rectified image outside dst_bytes,
 *     two rectified images that share a byte, src and dst ranges that share a byte, a fill above 0xFFFFFF, a parameter that
 *     is not finite, a focal length <= 0 or above CODETR_UNDISTORT_MAX_FOCAL, a centre beyond CODETR_UNDISTORT_MAX_CENTRE;
 *     CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX or a side above CODETR_FRAME_MAX_SIDE.
 */
#ifndef CODETR_UNDISTORT_H_
#define CODETR_UNDISTORT_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_UNDISTORT_ABI_VERSION 1
#define CODETR_UNDISTORT_BROWN 0
#define CODETR_UNDISTORT_FISHEYE 1
#define CODETR_UNDISTORT_ROW_INTS 9
#define CODETR_UNDISTORT_PARAM_FLOATS 16
#define CODETR_UNDISTORT_MAX_FOCAL 16384
#define CODETR_UNDISTORT_MAX_CENTRE 32768

int codetr_undistort_abi_version(void);
int codetr_undistort_rgb_u8(void *stream, const void *src_dev, int64_t src_bytes, int64_t N, const int64_t *rows_host,
                            const float *params_host, void *dst_dev, int64_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_UNDISTORT_H_ */
