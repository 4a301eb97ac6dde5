/* C ABI of libsrgd_consistency.so: LR consistency (LR-PSNR) of a x4 super-resolved image against its own low-resolution input on
 * the MI355X (gfx950).  Engine-free: raw device pointers and sizes, no engine handle, no torch types.  A library of its own beside
 * libsrgd_hip.so (include/srgd_hip.h), libsrgd_metrics.so (include/srgd_metrics.h) and libsrgd_ensemble.so (include/srgd_ensemble.h),
 * built by the same srgd_amd/build.py from srgd_amd/csrc/consistency.hip: none of their export tables changes. */
#ifndef SRGD_CONSISTENCY_H
#define SRGD_CONSISTENCY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_image_consistency_last_error(void);

/* The five coefficient vectors that describe the x4 reduction of every image with h, w >= 5 (host only, no GPU): out[0] = output
 * index 0 (10 taps from input index 0), out[1] = index 1 (14 taps from 0), out[2] = every interior index i in 2 .. n-3 (16 taps from
 * 4*i - 6), out[3] = index n-2 (14 taps from 4*n - 14), out[4] = index n-1 (10 taps from 4*n - 10); each begins at its first tap and
 * is zero beyond its last.  Computed by Pillow's precompute_coeffs formula (below); none depends on n.  Returns 0, or -1 for NULL. */
int srgd_image_consistency_coeffs(int32_t out[5][16]);

/* LR consistency of one image (engine extension, absent upstream): does the output, reduced by the scale factor with the operator
 * that made the condition, still explain the input?  Inputs and outputs are 8-bit, so every result is an exact integer.
 * Definition.  L is the input as decoded, uint8 [h][w][3].  O is the output AS SAVED (after --color_fix), uint8 [4h][4w][3].
 *   D = Pillow Image.resize((w, h), BICUBIC) of O, exactly as src/libImaging/Resample.c computes it:
 *     coefficients from precompute_coeffs: support 2.0 * 4 = 8, a = -0.5, window clipped to the image and renormalised, 22-bit
 *       fixed point, round half away from zero;
 *     horizontal pass over all 4h rows, accumulator 1 << 21, result clip8(acc >> 22), rounded to 8 bits;
 *     then the vertical pass on that result, the same way.
 *   e = D - L per element.  stats, four int64:  sse_r, sse_g, sse_b = sum of e^2 per channel,  max_abs = max |e|.
 *   The host derives in float64:  lr_mse = (sse_r + sse_g + sse_b) / (3*h*w),  lr_psnr = 10*log10(255^2 / lr_mse) (+inf at 0),
 *   lr_max_abs = max_abs.
 * down_u8 (optional, NULL = not written): D, uint8 [h][w][3].
 * Work split.  The image is cut into tiles of 32 x 15 LR pixels (width x height), one workgroup each; a tile's record {sse_r, sse_g,
 * sse_b, max_abs} (4 x 8 bytes) is stored plainly and a second kernel, one workgroup per image, adds the records.  All integers, no
 * atomics; the ownership of pixels by tiles depends on (h, w) alone.
 * Layout.  hr_u8 is 16-byte aligned (a row of O is read with 16-byte loads where w % 4 == 0, with guarded 4-byte loads otherwise),
 * stats and scratch are 8-byte aligned; lr_u8 and down_u8 are read and written byte by byte and need no alignment.  Nothing outside
 * the 3*h*w bytes of down_u8 and the four int64 of stats is ever written.
 * scratch: device memory owned by the caller, 32 * ceil(h / 15) * ceil(w / 32) bytes (one record per tile).
 * Errors (-1, nothing is launched, nothing is written; the message: srgd_image_consistency_last_error()): a null pointer other than
 * down_u8, h or w < 5 (the clipped windows then overlap and depend on the size), 48*h*w >= 2^31 - 256, a misaligned pointer.
 * Two launches.  Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_image_consistency(const uint8_t* hr_u8, const uint8_t* lr_u8, int h, int w, uint8_t* down_u8, int64_t* stats, void* scratch,
                           void* stream);
/* srgd_image_consistency for n_images >= 1 images held in flat buffers.  hw_host = h_0, w_0, h_1, w_1, ... (the LR sizes); image i's
 * output O begins at byte hr_offsets_host[i] of hr_u8, its input L at byte lr_offsets_host[i] of lr_u8, its D at byte
 * down_offsets_host[i] of down_u8 (down_u8 and down_offsets_host are NULL together); stats: device int64 [n_images][4] = sse_r,
 * sse_g, sse_b, max_abs.  All offsets are multiples of 16 in [0, 2^36) - anything else is an error before any launch.
 * One launch sequence (two launches) covers up to 128 images (the grid's y index is the image, its record travels as a kernel
 * argument; a larger group runs as consecutive sequences of 128).  Every byte of D and the four integers of an image are
 * bit-identical to srgd_image_consistency on that image alone, in any group and at any offsets.  Every image is checked before the
 * first launch: on an error nothing is written.
 * scratch: sum_i 32 * ceil(h_i / 15) * ceil(w_i / 32) bytes. */
int srgd_image_consistency_images(const uint8_t* hr_u8, const int64_t* hr_offsets_host, const uint8_t* lr_u8,
                                  const int64_t* lr_offsets_host, const int32_t* hw_host, int n_images, uint8_t* down_u8,
                                  const int64_t* down_offsets_host, int64_t* stats, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
