/* C ABI of libsrgd_guidance.so: LR-consistency guidance of the tiled DDPM sampler on the MI355X (gfx950) - after a sampling step, the
 * model's prediction of the clean image (x_start) is pulled towards the low-resolution input it is conditioned on, and the image
 * canvas receives the same correction scaled by the posterior mean's weight of x_start.  Engine-free: raw device pointers, a host
 * record array and a caller-owned scratch; no engine handle, no torch types.  A library of its own beside libsrgd_hip.so
 * (include/srgd_hip.h), libsrgd_metrics.so, libsrgd_ensemble.so, libsrgd_consistency.so and libsrgd_backproject.so, built by the same
 * srgd_amd/build.py from srgd_amd/csrc/guidance.hip: none of their export tables changes. */
#ifndef SRGD_GUIDANCE_H
#define SRGD_GUIDANCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One image of a call: its [3][Hp][Wp] fp32 canvas begins at element canvas_off of img and of x_start alike, its condition
 * [3][4h][4w] fp32 in [0,1] at element cond_off of cond01.  The crop box is rows top .. top + 4h, columns left .. left + 4w of every
 * canvas plane; h x w is the size of the low-resolution input. */
typedef struct srgd_guidance_image {
  int64_t canvas_off;
  int64_t cond_off;
  int32_t Hp, Wp, top, left, h, w;
} srgd_guidance_image;

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_guidance_last_error(void);

/* The coefficient vectors of the two operators as the kernels use them (host only, no GPU), every one an integer of Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc for bicubic divided by 2^22 (exact in fp32; the integers of a row sum to 2^22 - 1, 2^22
 * or 2^22 + 1, so a row sums to 1 within 2^-22).
 * down[v][t]: the reduction 4n -> n, n >= 5, laid on the frame [4i - 6, 4i + 10) of output i: v = 0, 1 for i = 0, 1; v = 2 for every i
 *   in 2 .. n-3; v = 3, 4 for i = n-2, n-1; taps of the frame outside the line are 0 (Pillow clips the window there and
 *   renormalises).  The integers srgd_image_consistency* and srgd_image_backproject* reduce with.
 * up[v][t]: the enlargement n -> 4n laid on the frame [floor((j - 6) / 4), + 4) of output j: v = j for j in 0 .. 5; v = 6 + (j - 6) % 4
 *   for j in 6 .. 4n-7; v = 10 + j - (4n - 6) for j in 4n-6 .. 4n-1; taps outside the line are 0.  The sixteen vectors of
 *   srgd_image_backproject_coeffs, each moved onto its frame.
 * Returns 0, or -1 for NULL. */
int srgd_guidance_coeffs(float down[5][16], float up[16][4]);

/* One guidance step on n_images >= 1 images (engine extension, absent upstream).  Per image, with H = 4h, W = 4w, per plane:
 *   X = x_start inside the crop box, [H][W].
 *   C = 2 * cond01 - 1 (fmaf(2, cond01, -1)).
 *   D(X), [h][w]: horizontal pass T[y][i] = sum_t down[v(i)][t] * X[y][4i - 6 + t] over the H rows, then the vertical pass
 *     D[i][x] = sum_t down[v(i)][t] * T[4i - 6 + t][x]; t ascending from an accumulator of 0, one fmaf per tap, fp32.  No 8-bit
 *     rounding and no clipping in between or after.
 *   U(D), [H][W]: horizontal pass S[y][j] = sum_t up[v(j)][t] * D[y][floor((j - 6) / 4) + t] over the h rows, then the vertical pass
 *     the same way; fp32, fmaf, t ascending.
 *   g = C - U(D(X));  x_start = fmaf(weight_x0, g, x_start);  img = fmaf(weight_img, g, img), inside the crop box only.
 * Everything outside the crop boxes keeps its bytes.  There are no clamps: an element where X is NaN or Inf comes out non-finite in
 * both canvases, and so does every element whose U(D(.)) reads it - at most 16 pixels away along either axis; all others are
 * untouched by it.
 * With the DDPM posterior mean alpha_next * (x_t * (1 - c) / alpha + c * x0), linear in x0, weight_img = gamma * alpha_next * c applies
 * to the canvas the correction weight_x0 = gamma applies to x0.
 * Work split.  Two launches per call and per 128 images: a reduce kernel (one workgroup per plane and tile of 32 x 15 LR pixels: the HR
 * patch of the tile, 72 rows x 144 columns of x_start, staged in LDS; writes D to the scratch) and an enlarge-and-update kernel
 * (the same tiles = 128 x 60 HR pixels: D with a halo of 2 staged in LDS; a workgroup reads x_start and img only at the elements it
 * writes).  The grid's y index is the image, its z index the plane; the records travel as a kernel argument.  No atomics: every
 * element depends on its own image's elements alone, so every image comes out bit-identical to the call on that image alone, in any
 * group and at any offsets.
 * Layout.  img, x_start and cond01 are 4-byte aligned, scratch is 256-byte aligned.  The canvases of a call are pairwise disjoint;
 * the elements the call covers in img, x_start, cond01 and the scratch do not overlap each other.  3*Hp*Wp < 2^31.
 * scratch: device memory owned by the caller, sum_i roundup(12*h_i*w_i, 256) bytes (D of image i, [3][h_i][w_i] fp32, in image order).
 * Errors (-1, nothing is launched, nothing is written; the message: srgd_guidance_last_error()): a null pointer, n_images < 1, h or
 * w < 5, a crop box that leaves its canvas, a negative offset, 3*Hp*Wp >= 2^31, a weight that is NaN or Inf, a misaligned pointer,
 * overlapping canvases or buffers.  Every image is checked before the first launch.
 * Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_guidance_step(float* img, float* x_start, const float* cond01, const srgd_guidance_image* images_host, int n_images,
                       float weight_x0, float weight_img, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
