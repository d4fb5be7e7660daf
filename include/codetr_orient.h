/* codetr_orient.h -- companion header of codetr_hip.h: EXIF orientations applied to the packed RGB uint8 images every
 * kernel of the Inferencer reads -- the eight flips / rotations / transposes of a stored image into the upright one -- and
 * the host reader of a JPEG file's orientation tag.  Exported from the same libcodetr_hip.so, versioned on its own.  Error
 * codes and the limits CODETR_PREPROCESS_BATCH_MAX / CODETR_FRAME_MAX_SIDE are codetr_hip.h's.
 *
 * The rule.  An orientation o is EXIF's 1..8 (tag 0x0112).  The stored image is H x W x 3, the upright one H' x W' x 3, and
 *   out[y'][x'][c] = in[y][x][c] for every 0 <= y < H, 0 <= x < W, c < 3 with
 *     o = 1: (y', x') = (y, x)              H', W' = H, W      as stored
 *     o = 2: (y', x') = (y, W-1-x)          H', W' = H, W      mirrored left to right
 *     o = 3: (y', x') = (H-1-y, W-1-x)      H', W' = H, W      turned by 180 degrees
 *     o = 4: (y', x') = (H-1-y, x)          H', W' = H, W      mirrored top to bottom
 *     o = 5: (y', x') = (x, y)              H', W' = W, H      transposed
 *     o = 6: (y', x') = (x, H-1-y)          H', W' = W, H      turned by 90 degrees clockwise
 *     o = 7: (y', x') = (W-1-x, H-1-y)      H', W' = W, H      transposed about the other diagonal
 *     o = 8: (y', x') = (W-1-x, y)          H', W' = W, H      turned by 90 degrees anticlockwise
 *   Bytes are copied, never computed: numpy's flips, rot90 and transposes and Pillow's ImageOps.exif_transpose give the
 *   same images.
 *
 * codetr_orient_rgb_u8: N <= CODETR_PREPROCESS_BATCH_MAX images in one launch (the caller splits).
 *   src_dev / src_bytes: one device buffer that holds every stored image, only read.
 *   rows_host: HOST [N][CODETR_ORIENT_ROW_INTS] int64: o, H, W, offset of the stored image in src_dev, its row pitch in
 *     bytes (>= 3 W; packed RGB, rows `pitch` apart), offset of the upright image in dst_dev.
 *   dst_dev / dst_bytes: image n is the packed H' x W' x 3 at its offset (row pitch 3 W'); bytes outside the images are not
 *     written.  src and dst are different buffers: there is no in-place form.
 *   One launch whatever the rows hold (csrc/orient.hip), no allocation, no synchronisation.  All checks run before any HIP
 *   call: CODETR_E_BADARG for a null pointer, N <= 0, a buffer size <= 0, an o outside 1..8, a side <= 0, a negative
 *     offset, a pitch below 3 W, a stored row outside src_bytes, an upright image outside dst_bytes, two upright images that
 *     share a byte, src and dst ranges that share a byte; CODETR_E_TOO_LARGE for N > CODETR_PREPROCESS_BATCH_MAX or a side
 *     above CODETR_FRAME_MAX_SIDE.
 *
 * codetr_orient_exif: HOST only, no HIP call.  The orientation a JPEG file asks for -> 1..8; CODETR_E_BADARG for a null
 *   pointer or bytes <= 0.  It never reads a byte outside [0, bytes).  Whatever the rule below does not name gives 1.
 *   The file starts FF D8.  From byte 2 the markers are walked: a position p needs p + 4 <= bytes and file[p] = FF; m =
 *   file[p+1].  m = FF is a fill byte (p += 1); m = 01 and D0..D7 stand alone (p += 2); m = DA (SOS) or D9 (EOI) ends the
 *   walk.  Any other marker has the big-endian length L = file[p+2..p+3], 2 <= L <= bytes - (p + 2), and the payload of L - 2
 *   bytes behind it; p += 2 + L.  The first APP1 (m = E1) whose payload has at least 6 bytes and starts "Exif\0\0" decides;
 *   no later segment is looked at.  The TIFF block t is the rest of that payload, T bytes, every offset below relative to
 *   it and every read inside [0, T): t[0..3] = "II*\0" (little-endian) or "MM\0*" (big-endian); d = the uint32 at 4 (the
 *   offset of IFD0); n = the uint16 at d; entry k < n is the 12 bytes at d + 2 + 12 k: tag (uint16), type (uint16), count
 *   (uint32), value.  The first entry with tag 0x0112 decides: type 3 (SHORT) and count 1 -> v = the uint16 at the entry's
 *   byte 8, in the block's byte order, returned when 1 <= v <= 8.
 */
#ifndef CODETR_ORIENT_H_
#define CODETR_ORIENT_H_

#include <stdint.h>

#include "codetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODETR_ORIENT_ABI_VERSION 1
#define CODETR_ORIENT_ROW_INTS 6

int codetr_orient_abi_version(void);
int codetr_orient_exif(const unsigned char *file_host, int64_t bytes);
int codetr_orient_rgb_u8(void *stream, const void *src_dev, int64_t src_bytes, int64_t N, const int64_t *rows_host,
                         void *dst_dev, int64_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CODETR_ORIENT_H_ */
