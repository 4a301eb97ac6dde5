/* C ABI of libsrgd_selfens.so: geometric self-ensemble (the "+" variant of the SR literature) on the MI355X (gfx950) - the eight
 * flips / rotations of an 8-bit RGB image, and the fused "turn every source back and average" of up to eight such images.
 * Engine-free: raw device pointers and sizes, no engine handle, no torch types.  A library of its own beside libsrgd_hip.so
 * (include/srgd_hip.h), libsrgd_metrics.so, libsrgd_ensemble.so, libsrgd_consistency.so, libsrgd_backproject.so, libsrgd_guidance.so,
 * libsrgd_solver.so, libsrgd_resize.so, libsrgd_alpha.so and libsrgd_threshold.so, built by the same srgd_amd/build.py from
 * srgd_amd/csrc/selfens.hip: none of their export tables changes.
 *
 * Definition.  A dihedral operation `op` in 0 .. 7 on an image x, uint8 [h][w][3]:
 *   bit 2: transpose (swap the two spatial axes); then bit 0: reverse the columns; then bit 1: reverse the rows.
 *   numpy:  x = x.swapaxes(0, 1) if op & 4 else x;  x = x[:, ::-1] if op & 1 else x;  x = x[::-1] if op & 2 else x
 * apply(x, op) is [h][w][3] for op < 4 and [w][h][3] for op >= 4.  inverse(op) = op for 0, 1, 2, 3, 4, 7; inverse(5) = 6,
 * inverse(6) = 5: apply(apply(x, op), inverse(op)) = x.
 * Merge.  n sources, 1 <= n <= 8; source j is apply(x_j, op_j) of some [H][W][3] image x_j, stored as [H][W][3] (op_j < 4) or
 * [W][H][3] (op_j >= 4).  Per byte, with S = sum_j apply(src_j, inverse(op_j)):
 *   m = (2*S + n) div (2*n)   (integer division: the nearest integer, halves up - the rule of include/srgd_ensemble.h's mean)
 *   mean01 (optional, NULL = not written), fp32 planar [3][H][W]:  (float)m / 255.0f, the merged image as ToTensor reads the PNG back.
 * The same op may appear more than once in a source list.
 *
 * Layout.  Images lie in flat uint8 device buffers at byte offsets that are multiples of 16 in [0, 2^36); rows are 3*w bytes,
 * unpadded, so a row starts at any byte; `src` and `dst` are 16-byte aligned, mean01 4-byte; mean01 offsets count floats, are
 * >= 0 and need no alignment.  3*h*w < 2^31 for every image.
 * Work split.  One workgroup of 256 threads owns a tile of 32 x 32 output pixels.  The tile's source rectangle of every source
 * (32 rows of at most 96 bytes, rows and columns exchanged for a transposing op) is read once, as runs of a source row: 16-byte
 * loads at 16-byte aligned addresses in the interior of a run, single bytes in front of the first and behind the last aligned
 * address, into an LDS tile of 32 rows x 116 bytes per source (SRGD_SELFENS_LDS_SOURCE = 3712 bytes; a row keeps its phase modulo
 * 16).  Transposition and the reversal of 3-byte pixels happen in the LDS reads: a thread owns 16 consecutive, 16-byte aligned bytes
 * of an output row, sums the sources in 32-bit registers (8 * 255 = 2040) and writes them with one 16-byte store, or byte by byte
 * where the row starts or ends inside them.  With mean01 the merged bytes go through a further 32 x 96 byte LDS tile and leave as
 * runs of floats of a plane's row, 16-byte stores at aligned addresses.  Every source byte is read once, every output byte written
 * once.  LDS: srgd_selfens_transform SRGD_SELFENS_LDS_TRANSFORM = 3712 bytes, srgd_selfens_merge SRGD_SELFENS_LDS_MERGE =
 * 8 * 3712 + 3072 = 32768 bytes.  No atomics, no reductions across threads: which thread owns which byte depends on the sizes alone,
 * so every byte (and float) of an image is identical to the call on that image alone, in any group and at any offsets.
 * The image index is the grid's y index and its record travels as a kernel argument: one launch (a launch sequence of one) covers
 * up to SRGD_SELFENS_MAX_IMAGES = 32 images, a larger group runs as consecutive launches of 32.
 * Errors: -1, nothing is launched, nothing is written, no pointer is touched; the message: srgd_selfens_last_error().  Every image
 * is checked on the host before the first launch.
 * Asynchronous on `stream`; no allocation, no synchronisation. */
#ifndef SRGD_SELFENS_H
#define SRGD_SELFENS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRGD_SELFENS_MAX_SOURCES 8       /* sources of one merged image */
#define SRGD_SELFENS_MAX_IMAGES 32       /* images of one launch */
#define SRGD_SELFENS_TILE 32             /* output pixels per side of a workgroup's tile */
#define SRGD_SELFENS_LDS_SOURCE 3712     /* LDS bytes of one source's tile: 32 rows x 116 */
#define SRGD_SELFENS_LDS_TRANSFORM 3712
#define SRGD_SELFENS_LDS_MERGE 32768     /* 8 x 3712 + 32 x 96 */

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_selfens_last_error(void);

/* One image of srgd_selfens_transform: the source [h][w][3] begins at byte src_off of `src`, the result apply(source, op) -
 * [h][w][3] for op < 4, [w][h][3] for op >= 4 - at byte dst_off of `dst`.  pad is ignored. */
typedef struct srgd_selfens_record {
  int64_t src_off, dst_off;
  int32_t h, w, op, pad;
} srgd_selfens_record;

/* dst = apply(src, op) for n >= 1 images of free sizes.  The inverse transform is the same entry with inverse(op).
 * Refused: a null pointer, n < 1, h or w < 1, 3*h*w >= 2^31, op outside 0 .. 7, an offset that is no multiple of 16 or lies outside
 * [0, 2^36), `src` or `dst` not 16-byte aligned, source images and destination images that overlap (the byte ranges from the first
 * to the last image of each side are compared). */
int srgd_selfens_transform(const void* src, void* dst, const srgd_selfens_record* records_host, int n, void* stream);

/* One image of srgd_selfens_merge: the merged [H][W][3] begins at byte dst_off of `dst_u8`, its three planes at element mean01_off
 * of `mean01` (ignored where mean01 is NULL); source j, j < n_src, begins at byte src_off[j] of `src`, is apply(x_j, op[j]) and is
 * stored [H][W][3] (op[j] < 4) or [W][H][3] (op[j] >= 4).  pad and the entries j >= n_src are ignored. */
typedef struct srgd_selfens_image {
  int64_t dst_off, mean01_off;
  int32_t H, W, n_src, pad;
  int64_t src_off[8];
  int32_t op[8];
} srgd_selfens_image;

/* The merge of every image of the batch, n_images >= 1, sizes and n_src free per image.
 * Refused: a null pointer other than mean01, n_images < 1, n_src outside 1 .. 8, H or W < 1, 3*H*W >= 2^31, an op outside 0 .. 7,
 * a byte offset that is no multiple of 16 or lies outside [0, 2^36), a negative mean01 offset (with mean01), `src` or `dst_u8` not
 * 16-byte aligned, mean01 not 4-byte aligned, source images and destination images that overlap (compared as in
 * srgd_selfens_transform). */
int srgd_selfens_merge(const void* src, void* dst_u8, float* mean01, const srgd_selfens_image* images_host, int n_images,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif
