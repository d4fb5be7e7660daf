/* codetr_jpeg.h -- companion header of codetr_hip.h: a baseline JPEG encoder for the images the drawing and frame
 * kernels leave on the device.  Exported from the same libcodetr_hip.so; versioned on its own (a self-contained addition
 * does not touch CODETR_HIP_ABI_VERSION).  Error codes and the limits CODETR_PREPROCESS_BATCH_MAX /
 * CODETR_DRAW_MAX_SIDE are codetr_hip.h's.
 *
 * Replaces the cv2.imwrite of the reference's Inferencer.visualize (codetr/inferencer.py:214-219), which writes
 * vis/%08d.jpg on the host.  The rule below is stated in integer arithmetic only, so that a restatement
 * (tests/jpeg_ref.py) reproduces the file byte for byte.  `>>` is an arithmetic shift (floor), `/` an integer division of
 * non-negative values.
 *
 * The file: baseline sequential JFIF (ITU T.81 SOF0, 8 bit, 3 components):
 *   SOI | APP0 "JFIF\0" 1.01, units 0, density 1:1, no thumbnail | DQT table 0 (luminance) | DQT table 1 (chrominance) |
 *   SOF0 | DHT DC 0 | DHT AC 0 | DHT DC 1 | DHT AC 1 | DRI | SOS | scan | EOI.
 *   Each DQT / DHT segment holds one table (8-bit DQT entries in zigzag order).  SOF0: precision 8, H, W, components
 *   1 (Y; sampling 2x2 at 4:2:0, 1x1 at 4:4:4; table 0), 2 (Cb; 1x1; table 1), 3 (Cr; 1x1; table 1).  SOS: components
 *   1 (DC 0 / AC 0), 2 and 3 (DC 1 / AC 1), Ss 0, Se 63, Ah/Al 0.  codetr_jpeg_header writes SOI..SOS, the kernels write
 *   the scan, the caller appends EOI (FF D9).
 *
 * Colour (full-range BT.601 as JFIF defines it; constants round(k * 2^16)), per pixel:
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11058 R - 21710 G + 32768 B + 8388608 + 32768) >> 16, then min(., 255)
 *   Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32768) >> 16, then min(., 255)
 *   (only pure blue / pure red reach 256; no value falls below 0).
 * Edge padding: the image is extended to a multiple of the MCU (16x16 at 4:2:0, 8x8 at 4:4:4) by repeating its last column
 *   and last row: pixel (x, y) reads (min(x, W - 1), min(y, H - 1)).
 * Subsampling 4:2:0: chroma sample = (a + b + c + d + 2) >> 2 over the Cb (Cr) of each 2x2 pixels.  MCU = Y blocks
 *   top-left, top-right, bottom-left, bottom-right, then Cb, then Cr.  4:4:4: MCU = Y, Cb, Cr of one 8x8.
 * Level shift and DCT: s = sample - 128.  C[k][n] = round(8192 * c(k) / 2 * cos((2n + 1) k pi / 16)), c(0) = 1/sqrt 2,
 *   c(k > 0) = 1, i.e. the rows
 *     k = 0:  2896  2896  2896  2896  2896  2896  2896  2896
 *     k = 1:  4017  3406  2276   799  -799 -2276 -3406 -4017
 *     k = 2:  3784  1567 -1567 -3784 -3784 -1567  1567  3784
 *     k = 3:  3406  -799 -4017 -2276  2276  4017   799 -3406
 *     k = 4:  2896 -2896 -2896  2896  2896 -2896 -2896  2896
 *     k = 5:  2276 -4017   799  3406 -3406  -799  4017 -2276
 *     k = 6:  1567 -3784  3784 -1567 -1567  3784 -3784  1567
 *     k = 7:   799 -2276  3406 -4017  4017 -3406  2276  -799
 *   Row pass, for every row y: t[y][u] = (sum_x C[u][x] s[y][x] + 512) >> 10 (three fraction bits kept);
 *   column pass: F[v][u] = (sum_y C[v][y] t[y][u] + 32768) >> 16.  int32 throughout (|row sum| < 2^22, |column sum| <
 *   2^27).  No residual scale: F is the T.81 coefficient.  |F| <= 1024, so the DC difference fits category 11 and an AC
 *   value category 10.
 * Quantisation: base = T.81 Annex K.1 (luminance for Y, chrominance for Cb / Cr); quality q in 1..100, the IJG rule:
 *   s = 5000 / q for q < 50, else 200 - 2 q; t = clamp((base * s + 50) / 100, 1, 255);
 *   coefficient c -> sign(c) * ((|c| + t / 2) / t).
 * Entropy coding: zigzag order; DC = difference to the previous block of the same component in the restart interval
 *   (0 before the first); the T.81 Annex K.3 tables (K.3 / K.5 for Y, K.4 / K.6 for Cb and Cr), as they are; a value v of
 *   category n = bit length of |v| is written as its n low bits, v - 1 for v < 0; ZRL (F0) for every full run of 16
 *   zeros in front of a non-zero coefficient; EOB (00) unless coefficient 63 is non-zero.
 * Restart intervals: DRI = MCUs per MCU row, so every MCU row is one interval: predictors reset, the row's bits padded
 *   with 1-bits to a byte, every FF data byte (pad bits included) followed by 00, then RSTm (FF D0+m), m = row mod 8,
 *   after every row but the last.
 *
 * codetr_jpeg_encode_u8: N <= CODETR_PREPROCESS_BATCH_MAX images (the caller splits), RGB uint8 HWC.
 *   buf_dev / buf_bytes / images_host: as codetr_draw_detections_* (HOST [N][3] int64: offset, H, W; sides 1 ..
 *     CODETR_DRAW_MAX_SIDE; inside the buffer; images may overlap here: they are only read).  No alignment asked.
 *   quality 1..100; subsampling CODETR_JPEG_420 / CODETR_JPEG_444.
 *   out_dev: image n's scan bytes start at n * out_stride (out_stride >= 1, the caller's choice; N * out_stride bytes);
 *   lengths_dev [N] int32: the scan's length, or -1 when it does not fit out_stride -- then nothing of that image is
 *     written, and never anything at or beyond a slot's end.  codetr_jpeg_scan_bound(H, W, subsampling) is a proven upper
 *     bound: 416 bytes per block (1660 bits: 22 of DC, 63 x 26 of AC, every byte stuffed) + 2 per RST marker.
 *   workspace_dev / workspace_bytes: at least codetr_jpeg_workspace_bytes(N, images_host, subsampling, out_stride)
 *     bytes, 16-byte aligned: int32 row lengths, then per MCU row min(416 * blocks of the row, out_stride) bytes rounded
 *     up to 16.
 *   Two launches, no host synchronisation (csrc/jpeg.hip): one 256-thread workgroup per MCU row encodes the row in passes
 *   of CODETR_JPEG_PASS_PIXELS pixels (28 MCUs at 4:2:0, 56 at 4:4:4) into the workspace; a second launch, again one
 *   workgroup per row, sums the row lengths of its image and copies its row and RST marker into the slot.
 *   CODETR_E_BADARG for a null pointer, N <= 0, an inconsistent row, quality or subsampling out of range,
 *   out_stride <= 0, a workspace that is too small or misaligned; CODETR_E_TOO_LARGE for
 *   N > CODETR_PREPROCESS_BATCH_MAX or a side > CODETR_DRAW_MAX_SIDE.  All checks run before any HIP call.
 * codetr_jpeg_workspace_bytes / codetr_jpeg_scan_bound: host only; a negative CODETR_E_* code for bad arguments.
 * codetr_jpeg_header: HOST only -- writes SOI up to and including SOS (CODETR_JPEG_HEADER_BYTES bytes) to out_host and
 *   returns that count; CODETR_E_BADARG for a null pointer, a side < 1 or > 65535 (SOF0 holds 16 bits; the encoder's own
 *   limit is lower), quality or subsampling out of range, capacity < CODETR_JPEG_HEADER_BYTES.
 */
#ifndef CODETR_JPEG_H_
#define CODETR_JPEG_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_JPEG_ABI_VERSION 1
#define CODETR_JPEG_420 0
#define CODETR_JPEG_444 1
#define CODETR_JPEG_HEADER_BYTES 629
#define CODETR_JPEG_PASS_PIXELS 448
#define CODETR_JPEG_BLOCK_BOUND 416

int codetr_jpeg_abi_version(void);
int codetr_jpeg_header(int64_t H, int64_t W, int quality, int subsampling, unsigned char *out_host, int64_t capacity);
int64_t codetr_jpeg_scan_bound(int64_t H, int64_t W, int subsampling);
int64_t codetr_jpeg_workspace_bytes(int64_t N, const int64_t *images_host, int subsampling, int64_t out_stride);
int codetr_jpeg_encode_u8(void *stream, const void *buf_dev, int64_t buf_bytes, int64_t N, const int64_t *images_host,
                          int quality, int subsampling, void *out_dev, int64_t out_stride, int *lengths_dev,
                          void *workspace_dev, int64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_JPEG_H_ */
