/* C ABI of libsrgd_alpha.so: what keeping the alpha channel of a transparent input needs on the MI355X (gfx950) - a Pillow-exact
 * resize of 8-bit planes, the interleave of an RGB image and a plane into RGBA, and the spread of visible colours into the
 * transparent area of an RGBA image ("alpha bleed").  Engine-free: raw device pointers and sizes, no engine handle, no torch types.
 * A library of its own beside libsrgd_hip.so (include/srgd_hip.h), libsrgd_metrics.so, libsrgd_ensemble.so, libsrgd_consistency.so,
 * libsrgd_backproject.so, libsrgd_guidance.so, libsrgd_solver.so and libsrgd_resize.so, built by the same srgd_amd/build.py from
 * srgd_amd/csrc/alpha.hip: none of their export tables changes.
 * Common to the three device entries: images lie in flat uint8 device buffers at byte offsets that are multiples of 16 in
 * [0, 2^36); the image index is the grid's y index and its record travels as a kernel argument, so one launch sequence covers up to
 * 128 images and a larger group runs as consecutive sequences of 128; all integers, vector loads and stores, no atomics; which
 * thread owns which output byte depends on the sizes alone, so every byte of an image's result is identical to the call on that
 * image alone, in any group and at any offsets; every image is checked on the host before the first launch.
 * Errors: -1, nothing is launched, nothing is written; the message: srgd_alpha_last_error().  Every buffer pointer is 16-byte
 * aligned (a misaligned one is refused like a null one).
 * Asynchronous on `stream`; no allocation, no synchronisation. */
#ifndef SRGD_ALPHA_H
#define SRGD_ALPHA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRGD_ALPHA_MAX_SIDE 16384     /* every size, in and out (SRGD_RESIZE_MAX_SIDE) */
#define SRGD_ALPHA_MAX_RATIO 8        /* plane resize, per axis: in <= 8 * out and out <= 8 * in (SRGD_RESIZE_MAX_RATIO) */
#define SRGD_ALPHA_MAX_TAPS 49        /* the widest row of a table (SRGD_RESIZE_MAX_TAPS) */
#define SRGD_ALPHA_MAX_BLEED 64       /* passes of srgd_alpha_bleed */

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_alpha_last_error(void);

/* One plane of srgd_alpha_resize_planes.  Plane i's source [h_in][w_in] begins at byte src_off of `src`, its result [h_out][w_out]
 * at byte dst_off of `dst`, its tables at byte tab_off of `tables`, laid out as include/srgd_resize.h lays them out: the table
 * w_in -> w_out where w_in != w_out, directly followed by the table h_in -> h_out where h_in != h_out; a table is int32
 * bounds[out][2] directly followed by int32 coeffs[out][ksize], as srgd_resize_coeffs of libsrgd_resize.so fills them.  This library
 * has no table code: k_h and k_v are the ksize of the two tables as srgd_resize_ksize returns it (1 .. 49; ignored where the pass
 * is skipped). */
typedef struct srgd_alpha_plane {
  int64_t src_off, dst_off, tab_off;
  int32_t h_in, w_in, h_out, w_out, k_h, k_v;
} srgd_alpha_plane;

/* Resize n_planes >= 1 uint8 planes.  With the tables of a filter of include/srgd_resize.h the result is
 * PIL.Image.resize((w_out, h_out), FILTER) of the mode-"L" image, bit for bit, which is also band A of that resize of an RGBA image:
 * the horizontal pass over all h_in rows, out[y][xx] = clip8(((1 << 21) + sum_x k[xx][x] * in[y][xmin + x]) >> 22), stored as 8 bits
 * [h_in][w_out] in `scratch`, then the vertical pass on that result.  A pass whose in == out is skipped; when both are skipped the
 * plane is copied.  `scratch` is device memory owned by the caller: plane i's part follows the part of plane i-1, each rounded up to
 * a multiple of 16 bytes, so scratch_bytes >= sum_i roundup(h_in_i * w_out_i, 16).
 * Work split.  Two kernels.  Horizontal: one workgroup of 256 threads per tile of 64 output pixels x 16 rows; the tile's bounds and
 * coefficient rows and the source span of its rows go to LDS, a thread owns one output pixel of four rows, the tile's result leaves
 * LDS as whole dwords.  Vertical: one workgroup per tile of 256 bytes x 16 output rows; a thread owns one dword of a row (lanes
 * along the contiguous byte axis) and walks the source rows of its window.  Rows of w bytes with w % 4 != 0 are not dword aligned:
 * such planes take a guarded byte path.  Every index read from a table is clamped to the plane before use: no table content makes a
 * kernel read or write outside its plane.  No byte outside the h_out * w_out bytes of each destination (and the scratch) is written.
 * Refused: a null pointer, n_planes < 1, a size outside 1 .. 16384, a ratio above 8, k_h or k_v outside 1 .. 49 where its pass
 * runs, an offset that is no multiple of 16 or lies outside [0, 2^36), `scratch` or `tables` not 16-byte aligned, tables_bytes or
 * scratch_bytes too small for the planes, source and destination planes that overlap. */
int srgd_alpha_resize_planes(const void* src, void* dst, const srgd_alpha_plane* planes_host, int n_planes, const void* tables,
                             int64_t tables_bytes, void* scratch, int64_t scratch_bytes, void* stream);

/* One image of srgd_alpha_pack_rgba and srgd_alpha_bleed: h x w pixels; its colour at byte rgb_off of the RGB buffer, its plane at
 * byte a_off of the plane buffer (pack only), its four-byte pixels at byte rgba_off of the RGBA buffer. */
typedef struct srgd_alpha_image {
  int64_t rgb_off, a_off, rgba_off;
  int32_t h, w;
} srgd_alpha_image;

/* Interleave: rgba[y][x] = (rgb[y][x][0], rgb[y][x][1], rgb[y][x][2], alpha[y][x]) for n_images >= 1 images - what
 * Image.merge("RGBA", (*rgb.split(), alpha)) holds.  An image is a flat run of h * w pixels; a thread owns 4 consecutive pixels:
 * three dword loads of colour, one of alpha, one 16-byte store, all aligned whatever w is; the last h * w % 4 pixels go byte by byte.
 * Refused: a null pointer, n_images < 1, a size outside 1 .. 16384, an offset that is no multiple of 16 or lies outside [0, 2^36),
 * destination images that overlap the colour or the planes. */
int srgd_alpha_pack_rgba(const void* rgb, const void* alpha, void* rgba, const srgd_alpha_image* images_host, int n_images,
                         void* stream);

/* Alpha bleed: RGBA [h][w][4] at rgba_off of `rgba` -> RGB [h][w][3] at rgb_off of `rgb` (a_off is ignored), `passes` in 0 .. 64.
 * The state is one RGB value and one `known` flag per pixel; initially known = (A > 0).  One pass reads only the state before the
 * pass: every pixel that is not known and has c >= 1 known pixels among its 8 neighbours inside the image gets, per channel,
 * (2 * s + c) / (2 * c) in integer division, s the sum over those c neighbours (their mean, rounded half up), and becomes known;
 * all other pixels keep their value.  After the last pass the RGB of the state is written: pixels still unknown keep their original
 * colour, known pixels never change, the alpha is not part of the result.  passes = 0 drops the fourth byte.
 * One launch per pass over two buffers of one dword per pixel (R, G, B, known) in `scratch`, then one launch that writes the three
 * bytes; no host round-trip in between.  `scratch` is device memory owned by the caller, 16-byte aligned:
 * scratch_bytes >= 2 * sum_i roundup(4 * h_i * w_i, 16) where passes > 0 (it is not touched where passes == 0).
 * Refused: a null pointer, n_images < 1, passes outside 0 .. 64, a size outside 1 .. 16384, an offset that is no multiple of 16 or
 * lies outside [0, 2^36), `scratch` not 16-byte aligned, scratch_bytes too small, source and destination images that overlap. */
int srgd_alpha_bleed(const void* rgba, void* rgb, const srgd_alpha_image* images_host, int n_images, int passes, void* scratch,
                     int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
