/* C ABI of libsrgd_resize.so: Pillow-exact resize of 8-bit RGB images by any ratio up to 8 either way on the MI355X (gfx950).
 * Engine-free: raw device pointers and sizes, no engine handle, no torch types.  A library of its own beside libsrgd_hip.so
 * (include/srgd_hip.h), libsrgd_metrics.so, libsrgd_ensemble.so, libsrgd_consistency.so, libsrgd_backproject.so, libsrgd_guidance.so
 * and libsrgd_solver.so, built by the same srgd_amd/build.py from srgd_amd/csrc/resize.hip: none of their export tables changes. */
#ifndef SRGD_RESIZE_H
#define SRGD_RESIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The filters, numbered as PIL.Image.Resampling numbers them. */
#define SRGD_RESIZE_LANCZOS 1  /* sinc(x) * sinc(x / 3) on -3 <= x < 3, sinc(x) = sin(pi x) / (pi x), sinc(0) = 1; support 3 */
#define SRGD_RESIZE_BILINEAR 2 /* 1 - |x| on |x| < 1; support 1 */
#define SRGD_RESIZE_BICUBIC 3  /* a = -0.5: ((a + 2)|x| - (a + 3)) x^2 + 1 on |x| < 1, (((|x| - 5)|x| + 8)|x| - 4) a on |x| < 2; support 2 */

#define SRGD_RESIZE_MAX_SIDE 16384 /* every size, in and out */
#define SRGD_RESIZE_MAX_RATIO 8    /* per axis: in <= 8 * out and out <= 8 * in */
#define SRGD_RESIZE_MAX_TAPS 49    /* the widest row of a table: 2 * ceil(3 * 8) + 1 (lanczos at 8 : 1) */

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_resize_last_error(void);

/* Definition.  The result is PIL.Image.resize((w_out, h_out), FILTER) of an 8-bit RGB image [h_in][w_in][3], bit for bit, as
 * Pillow 12's src/libImaging/Resample.c computes it:
 * The table of an axis that goes from `in` samples to `out` (precompute_coeffs, normalize_coeffs_8bpc), all in double:
 *   scale = in / out;  filterscale = max(scale, 1);  support = filter_support * filterscale;  ksize = 2 * (int)ceil(support) + 1;
 *   for every output xx:  center = (xx + 0.5) * scale;  xmin = max((int)(center - support + 0.5), 0);
 *     count = min((int)(center + support + 0.5), in) - xmin;
 *     w[x] = filter((x + xmin - center + 0.5) * (1 / filterscale)) for x in 0 .. count-1;  ww = their sum, added left to right;
 *     each w[x] is divided by ww where ww != 0, then k[x] = (int)(w[x] * 2^22 + 0.5) for w[x] >= 0 and (int)(w[x] * 2^22 - 0.5)
 *     below (round half away from zero to 22-bit fixed point);  k[x] = 0 for x in count .. ksize-1.
 * The horizontal pass runs over all h_in rows: out[y][xx][c] = clip8(((1 << 21) + sum_x k[xx][x] * in[y][xmin + x][c]) >> 22), an
 *   arithmetic shift, clip8 = clamp to 0 .. 255; the result is stored as 8 bits [h_in][w_out][3].
 * The vertical pass then runs on that 8-bit result in the same way, with the table of h_in -> h_out.
 * A pass whose in == out is skipped; when both are skipped the image is copied.
 * Accumulators are int32 as Pillow's, products are taken modulo 2^32.  The largest sum of |k| * 255 over all tables within the ratio
 * limit (lanczos at 8 : 1) measures 0.77 * 2^31: nothing overflows. */

/* ksize of the table in_size -> out_size (host only, no GPU).  -1: a size outside 1 .. 16384, a ratio above 8, an unknown filter. */
int srgd_resize_ksize(int in_size, int out_size, int filter);

/* The table in_size -> out_size (host only, no GPU; computed in double in the order above, compiled without floating-point
 * contraction): bounds[out_size][2] = (xmin, count) and coeffs[out_size][ksize], zero from count on.  Returns 0, or -1 for NULL and
 * for what srgd_resize_ksize refuses. */
int srgd_resize_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coeffs);

/* One image of a call.  Image i's source [h_in][w_in][3] begins at byte src_off of `src`, its result [h_out][w_out][3] at byte
 * dst_off of `dst`, its tables at byte tab_off of `tables`: the table w_in -> w_out where w_in != w_out, directly followed by the
 * table h_in -> h_out where h_in != h_out; a table is int32 bounds[out][2] directly followed by int32 coeffs[out][ksize], as
 * srgd_resize_coeffs fills them.  The three offsets are multiples of 16 in [0, 2^36). */
typedef struct srgd_resize_image {
  int64_t src_off, dst_off, tab_off;
  int32_t h_in, w_in, h_out, w_out;
} srgd_resize_image;

/* Resize n_images >= 1 images held in flat uint8 device buffers.  `tables` is a device buffer of tables_bytes bytes that the caller
 * filled (srgd_resize_coeffs, then an upload); `scratch` is device memory owned by the caller that receives the horizontal pass:
 * image i's part [h_in][w_out][3] follows the part of image i-1, each rounded up to a multiple of 16 bytes, so
 * scratch_bytes >= sum_i roundup(3 * h_in_i * w_out_i, 16).
 * Accepted geometry, per axis: 1 <= in, out <= 16384, in <= 8 * out, out <= 8 * in (at most 49 taps).
 * Work split.  Two kernels.  The horizontal pass: one workgroup of 256 threads per tile of 32 output pixels x 16 rows; the tile's
 * bounds and coefficient rows and the source span of its rows go to LDS, a thread owns one output pixel of two rows, the tile's
 * result leaves LDS as whole dwords.  The vertical pass: one workgroup per tile of 256 bytes x 16 output rows; the tile's bounds and
 * coefficient rows go to LDS, a thread owns one dword of a row (lanes along the contiguous byte axis) and walks the source rows of
 * its window.  Rows of 3 * w bytes with w % 4 != 0 are not dword aligned: such images take a guarded byte path.  Where the vertical
 * pass is skipped the horizontal pass writes the destination; where both are skipped the vertical kernel copies.  The image index is
 * the grid's y index, its record travels as a kernel argument: one launch sequence (at most 2 launches) covers up to 128 images, a
 * larger group runs as consecutive sequences of 128.  All integers, vector loads and stores, no atomics; the ownership of pixels by
 * tiles depends on the sizes alone, so every byte of an image's result is identical to the call on that image alone, in any group
 * and at any offsets.  No byte outside the 3 * h_out * w_out bytes of each destination image (and the scratch) is written.
 * Errors (-1, nothing is launched, nothing is written; the message: srgd_resize_last_error()) - every image is checked before the
 * first launch: a null pointer, n_images < 1, a size outside 1 .. 16384, a ratio above 8, an offset that is no multiple of 16 or
 * lies outside [0, 2^36), an unknown filter, `scratch` or `tables` not 16-byte aligned, tables_bytes or scratch_bytes too small for
 * the images, source and destination images that overlap.
 * Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_resize_u8_images(const void* src, void* dst, const srgd_resize_image* images_host, int n_images, int filter,
                          const void* tables, int64_t tables_bytes, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
