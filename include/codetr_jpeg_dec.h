/* codetr_jpeg_dec.h -- companion header of codetr_hip.h: a baseline JPEG decoder that leaves packed RGB uint8 images on
 * the device, where every later kernel of the Inferencer reads them.  The input-side mirror of codetr_jpeg.h; exported
 * from the same libcodetr_hip.so, versioned on its own.  Error codes and the limits CODETR_PREPROCESS_BATCH_MAX /
 * CODETR_FRAME_MAX_SIDE are codetr_hip.h's.
 *
 * The reference's Inferencer.__call__ takes decoded arrays only; the arithmetic matched here is libjpeg's (jidctint
 * "islow", fancy upsampling, jdcolor), as Pillow runs it.  The rule is stated in integer arithmetic only, so that a
 * restatement (tests/jpeg_dec_ref.py) reproduces every byte.  `>>` is an arithmetic shift, `/` a division of
 * non-negative integers; int32 arithmetic wraps in two's complement.
 *
 * Supported files: baseline sequential DCT (SOF0, 8 bit, Huffman), one interleaved scan with Ss 0, Se 63, Ah/Al 0, 8-bit
 *   quantiser tables, any DHT tables, any DRI; one component (grey, R = G = B; its sampling factors are taken as 1x1) or
 *   three components taken as Y/Cb/Cr with chroma sampling 1x1 and luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0).  APPn and
 *   COM are skipped (EXIF orientation is not applied); bytes after the last EOI are ignored.
 *
 * codetr_jpegdec_parse: HOST only, no HIP call.  Reads the markers from SOI up to and including SOS and finds the last
 *   FF D9 of the file; the scan is what lies between (stuffed, with its RSTm markers).
 *   info_host  [CODETR_JPEGDEC_INFO_INTS] int32: 0 H, 1 W, 2 components, 3 restart interval (MCUs, 0 = none),
 *     4 scan offset in the file, 5 scan bytes, 6 reason (a CODETR_JPEGDEC_R_*; 0 when supported), 7 hmax, 8 vmax,
 *     9 + 5 c .. 13 + 5 c for component c < 3: h, v, quantiser table, DC table, AC table,
 *     24 MCUs per row, 25 MCU rows, 26 blocks per MCU, 27 blocks of the scan, 28 .. 31 zero.
 *   tables_host [CODETR_JPEGDEC_TABLE_BYTES] bytes: quantiser tables 0..3, 64 bytes each in natural (de-zigzagged) order;
 *     then DC tables 0..3 and AC tables 0..3, each BITS[16] then HUFFVAL[256] (T.81 B.2.4.2); a table the file does not
 *     define is zero.
 *   Returns 0, or CODETR_E_BADARG for a null pointer or a malformed header (no SOI, a segment that runs outside the file,
 *     a table that is referenced but missing, DHT counts above 256 or codes that overflow their length, a zero dimension,
 *     SOS components that are not the frame's, no FF D9 behind SOS), CODETR_E_TOO_LARGE for a side above
 *     CODETR_FRAME_MAX_SIDE or a file of 2^27 bytes or more, CODETR_E_UNSUPPORTED with info[6] set for a well-formed
 *     file outside the supported set.  When several reasons hold the lowest-numbered one is reported.  H, W and the
 *     component count are filled in whenever SOF was read.
 *
 * Entropy decoding (T.81 F.2.2).  Bits are read MSB first; a data byte FF is followed by a stuffed 00 that is skipped.
 *   A position is (p, b): raw byte p of the scan holds the next bit, b of its bits are consumed; after the last bit of a
 *   byte p moves to the next data byte.  A Huffman code is matched by the canonical rule of F.2.2.3 against the next 16
 *   bits.  Any FF that is not followed by 00, and the end of the scan, stop the reader: bits behind it read as 0 and are
 *   not available.
 *   One step decodes one symbol of block `blk` of the MCU (component comp[blk]) at zigzag index k:
 *     no code matches and 16 bits are available              -> CODETR_JPEGDEC_S_BAD_CODE, the decode ends;
 *     no code matches with fewer bits, or code + value bits reach past the available bits -> the reader was stopped:
 *       by FF D0..D7 -> CODETR_JPEGDEC_S_RST, then restart behind that marker (below); by anything else ->
 *       CODETR_JPEGDEC_S_EXHAUSTED, the decode ends;
 *     k = 0: the DC symbol is the category s (s > 15 -> CODETR_JPEGDEC_S_DC_CATEGORY, the decode ends), then s bits v,
 *       EXTEND (F.2.2.1): v < 2^(s-1) -> v - 2^s + 1.  pred[comp] += v in int32; the stored coefficient 0 is pred
 *       saturated to int16.  k becomes 1.
 *     k > 0: the AC symbol is RRRRSSSS.  SSSS = 0: RRRR = 15 (ZRL) -> k += 16; any other RRRR is EOB and completes the
 *       block.  SSSS > 0: k += RRRR, coefficient zigzag[k] = EXTEND(SSSS bits), k += 1; k = 64 completes the block.
 *       An index above 63 where a coefficient (or, after ZRL, a further symbol) has to go ->
 *       CODETR_JPEGDEC_S_INDEX, the decode ends.
 *   A block is 64 int16 in natural order, zero where nothing was coded.  Blocks follow in MCU order: per MCU, per
 *   component, v rows of h blocks.  After the last block of an MCU: when the next data byte position (behind the rest of
 *   a partly consumed byte, whose bits are padding) holds FF D0+m, the decoder restarts: p behind the marker, b = 0, all
 *   predictors 0.  With M MCUs complete and fewer than all: a restart is expected exactly when DRI > 0 and M % DRI = 0; an
 *   unexpected one -> CODETR_JPEGDEC_S_INTERVAL, a wrong m (not (M / DRI - 1) % 8) or an expected one that is missing ->
 *   CODETR_JPEGDEC_S_RST; the decode goes on either way.  The status of an image is the first of these in scan order,
 *   0 when there is none; whatever happens behind the last block of the image is ignored.
 * Dequantisation: c * q in int32.
 * IDCT: libjpeg's jidctint, CONST_BITS 13, PASS1_BITS 2.  One 1-D pass over v[0..7]:
 *     z1 = (v2 + v6) * 4433; t2 = z1 - v6 * 15137; t3 = z1 + v2 * 6270; t0 = (v0 + v4) << 13; t1 = (v0 - v4) << 13;
 *     t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2;
 *     a0 = v7, a1 = v5, a2 = v3, a3 = v1; z1 = a0 + a3; z2 = a1 + a2; z3 = a0 + a2; z4 = a1 + a3; z5 = (z3 + z4) * 9633;
 *     a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5;
 *     z4 = z4 * -3196 + z5; a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
 *     out 0..7 = t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3, each (x + (1 << (s-1))) >> s.
 *   First over the columns with s = 11, then over the rows with s = 18; sample = clamp(value + 128, 0, 255).
 * Chroma upsampling (libjpeg's "fancy" rule) over the component's real sample grid, dw = ceil(W h_c / hmax) columns and
 *   dh = ceil(H v_c / vmax) rows:
 *   4:2:2, dw > 2: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2, out[0] = in[0],
 *     out[2 dw - 1] = in[dw - 1].
 *   4:2:0, dw > 2: s[i] = 3 in[r][i] + in[r-1][i] for output row 2r, 3 in[r][i] + in[r+1][i] for row 2r+1 (row -1 is row 0,
 *     row dh is row dh - 1); out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4,
 *     out[0] = (4 s[0] + 8) >> 4, out[2 dw - 1] = (4 s[dw-1] + 7) >> 4.
 *   dw <= 2: replication, out[y][x] = in[y / 2][x / 2] (in[y][x / 2] at 4:2:2).
 * Colour, cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *   B = Y + ((116130 cb + 32768) >> 16), each clamped to 0..255.  The image is the top-left H x W.
 *
 * codetr_jpegdec_decode_u8: N <= CODETR_PREPROCESS_BATCH_MAX files (the caller splits).
 *   scans_dev / scans_bytes: one device buffer with the files' scan bytes as they are in the file.
 *   rows_host: HOST [N][CODETR_JPEGDEC_ROW_INTS] int64: scan offset in scans_dev, scan bytes, H, W, offset of the image in
 *     dst_dev.  infos_host: HOST [N][CODETR_JPEGDEC_INFO_INTS] int32 as the parser wrote them (reason 0; H, W and scan
 *     bytes equal to the row's).  tables_dev: DEVICE [N][CODETR_JPEGDEC_TABLE_BYTES] as the parser wrote them.
 *   dst_dev / dst_bytes: image n is H x W x 3 uint8 at its offset; images must not overlap.  status_dev [N] int32: 0 or a
 *     CODETR_JPEGDEC_S_*; the pixels of a failed image are unspecified but stay inside its H * W * 3 bytes.
 *   workspace_dev / workspace_bytes: at least codetr_jpegdec_workspace_bytes(N, rows_host, infos_host), 16-byte aligned.
 *   Two memsets and five launches whatever the files hold, no host synchronisation, no allocation (csrc/jpeg_dec.hip):
 *   the scan is cut into chunks of CODETR_JPEGDEC_CHUNK_BYTES raw bytes, one lane per chunk, a lane owns the symbols
 *   that start in its chunk.  (1) one workgroup per run of CODETR_JPEGDEC_RUN_CHUNKS chunks: every lane decodes from the
 *   guess "first bit of the chunk, block 0, k 0", exit states become the next lanes' entry states and changed lanes
 *   decode again until nothing changes (at most one round per chunk; a lane behind a decode that ended keeps its
 *   guess, and only the final pass reports); (2) one workgroup per image repairs, in order, the
 *   runs whose guessed entry was wrong, then scans the chunks' block counts and DC sums; (3) every lane decodes once
 *   more from its now final state and writes coefficients and status; (4) dequantisation and IDCT into component
 *   planes; (5) upsampling and colour, one thread per pixel.
 *   CODETR_E_BADARG for a null pointer, N <= 0, a row that does not agree with its info or lies outside its buffer,
 *   overlapping images, a workspace that is too small or misaligned; CODETR_E_UNSUPPORTED for an info with a reason or
 *   outside the supported set; CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX or a side above
 *   CODETR_FRAME_MAX_SIDE.  All checks run before any HIP call.
 * codetr_jpegdec_workspace_bytes / codetr_jpegdec_output_bytes (H * W * 3 rounded up to 16): host only; a negative
 *   CODETR_E_* code for bad arguments.
 */
#ifndef CODETR_JPEG_DEC_H_
#define CODETR_JPEG_DEC_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_JPEGDEC_ABI_VERSION 1
#define CODETR_JPEGDEC_INFO_INTS 32
#define CODETR_JPEGDEC_ROW_INTS 5
#define CODETR_JPEGDEC_TABLE_BYTES 2432
#define CODETR_JPEGDEC_CHUNK_BYTES 64
#define CODETR_JPEGDEC_RUN_CHUNKS 256
#define CODETR_JPEGDEC_MAX_FILE_BYTES 134217727

#define CODETR_JPEGDEC_R_PROGRESSIVE 1
#define CODETR_JPEGDEC_R_EXTENDED 2
#define CODETR_JPEGDEC_R_LOSSLESS 3
#define CODETR_JPEGDEC_R_HIERARCHICAL 4
#define CODETR_JPEGDEC_R_ARITHMETIC 5
#define CODETR_JPEGDEC_R_PRECISION 6
#define CODETR_JPEGDEC_R_COMPONENTS 7
#define CODETR_JPEGDEC_R_RGB_IDS 8
#define CODETR_JPEGDEC_R_ADOBE 9
#define CODETR_JPEGDEC_R_SAMPLING 10
#define CODETR_JPEGDEC_R_QUANT16 11
#define CODETR_JPEGDEC_R_MULTISCAN 12
#define CODETR_JPEGDEC_R_SCAN_PARAMS 13

#define CODETR_JPEGDEC_S_BAD_CODE 1
#define CODETR_JPEGDEC_S_DC_CATEGORY 2
#define CODETR_JPEGDEC_S_INDEX 3
#define CODETR_JPEGDEC_S_EXHAUSTED 4
#define CODETR_JPEGDEC_S_RST 5
#define CODETR_JPEGDEC_S_INTERVAL 6

int codetr_jpegdec_abi_version(void);
int codetr_jpegdec_parse(const unsigned char *file_host, int64_t bytes, int32_t *info_host, unsigned char *tables_host);
int64_t codetr_jpegdec_output_bytes(int64_t H, int64_t W);
int64_t codetr_jpegdec_workspace_bytes(int64_t N, const int64_t *rows_host, const int32_t *infos_host);
int codetr_jpegdec_decode_u8(void *stream, const void *scans_dev, int64_t scans_bytes, int64_t N, const int64_t *rows_host,
                             const int32_t *infos_host, const void *tables_dev, void *dst_dev, int64_t dst_bytes,
                             int *status_dev, void *workspace_dev, int64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_JPEG_DEC_H_ */
