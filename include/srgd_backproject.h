/* C ABI of libsrgd_backproject.so: iterative back-projection of a x4 super-resolved image onto its own low-resolution input on the
 * MI355X (gfx950).  Engine-free: raw device pointers and sizes, no engine handle, no torch types.  A library of its own beside
 * libsrgd_hip.so (include/srgd_hip.h), libsrgd_metrics.so (include/srgd_metrics.h), libsrgd_ensemble.so (include/srgd_ensemble.h) and
 * libsrgd_consistency.so (include/srgd_consistency.h), built by the same srgd_amd/build.py from srgd_amd/csrc/backproject.hip: none
 * of their export tables changes. */
#ifndef SRGD_BACKPROJECT_H
#define SRGD_BACKPROJECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_image_backproject_last_error(void);

/* The sixteen coefficient vectors that describe the x4 enlargement of every line of n >= 5 samples to 4n (host only, no GPU):
 * out[0..5] = output indices 0 .. 5 (2, 2, 3, 3, 3, 3 taps from input index 0), out[6 + p] = every interior index j in 6 .. 4n-7 of
 * phase p = (j - 6) % 4 (4 taps from input (j - 6) / 4), out[10..15] = output indices 4n-6 .. 4n-1 (3, 3, 3, 3, 2, 2 taps that end at
 * input n-1); each begins at its first tap and is zero beyond its last.  Computed by Pillow's precompute_coeffs formula; none depends
 * on n.  Returns 0, or -1 for NULL. */
int srgd_image_backproject_coeffs(int32_t out[16][4]);

/* Iterative back-projection of one image (engine extension, absent upstream): the output is pulled back onto the input it was sampled
 * from with the two operators the project owns as Pillow-exact integer code.  Everything between the two quantisations is 8-bit, so
 * every result is an exact integer.
 * Inputs.  out01 and cond01 are fp32 planar [3][H][W], H = 4h, W = 4w, h, w >= 5, 48*h*w < 2^31 - 256; iterations = N, 1 <= N <= 64.
 * Quantising the output.  O_0 = q(out01), element-wise into uint8 [H][W][3]:  t = fmul_rn(v, 255);  q = 0 if t is NaN or t <= 0,
 *   q = 255 if t >= 255, otherwise q = (int)t, truncated.  On [0,1] this is srgd_image_unit_to_u8, the file as saved; outside [0,1]
 *   it saturates where the saved file wraps.
 * Quantising the condition.  C = r(cond01):  r = 0 for NaN, otherwise r = clamp((int)floorf(fmul_rn(v, 255) + 0.5f), 0, 255).  For a
 *   condition made by the front end, u8 / 255, this returns that u8 for all 256 values.
 * The iteration, for k = 1 .. N:
 *   D = Pillow Image.resize((w, h), BICUBIC) of O_{k-1}: word for word the D of include/srgd_consistency.h.
 *   U = Pillow Image.resize((W, H), BICUBIC) of D, exactly as src/libImaging/Resample.c computes it: support 2, a = -0.5, window
 *     clipped to the image and renormalised, 22-bit fixed point, round half away from zero; horizontal pass over the h rows to
 *     [h][W], accumulator 1 << 21, result clip8(acc >> 22), rounded to 8 bits; then the vertical pass on that result, the same way.
 *   O_k = clip(O_{k-1} + C - U, 0, 255), per element, in int.
 *   Where the condition was made from an input L, C - U is enlarge(L) - enlarge(D): the classic correction up to the 8-bit rounding
 *   of the two enlargements.
 * Result.  dst01 = fdiv_rn((float)O_N, 255), planar [3][H][W]: the tensor ToTensor of the saved file gives, and q(dst01) = O_N
 *   exactly.  Elements where out01 was non-finite receive out01's value unchanged: NaN and Inf stay visible.
 * Work split.  A begin kernel quantises out01 and cond01 into the scratch; every iteration is a reduce kernel (tiles of 32 x 15 LR
 * pixels, one workgroup each, writes D) and an update kernel (the same tiles = 128 x 60 HR pixels, O updated in place: a workgroup
 * reads O only at the elements it writes); an end kernel writes dst01.  2 + 2 N launches.  All integers, no atomics; the ownership of
 * pixels by tiles depends on (h, w) alone.
 * Layout.  out01, cond01 and dst01 are 4-byte aligned, scratch is 256-byte aligned.  dst01 == out01 is allowed and means in place; any
 * other overlap of dst01 with out01 or cond01 is an error.  Nothing outside the 48*h*w floats of dst01 and the scratch is written.
 * scratch: device memory owned by the caller, per image O (48*h*w bytes) + C (48*h*w bytes) + D (3*h*w bytes), each rounded up to a
 * multiple of 256 bytes.
 * Errors (-1, nothing is launched, nothing is written; the message: srgd_image_backproject_last_error()): a null pointer, iterations
 * outside 1 .. 64, h or w < 5, 48*h*w >= 2^31 - 256, a misaligned pointer, partial overlap.
 * Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_image_backproject(const float* out01, const float* cond01, int h, int w, int iterations, float* dst01, void* scratch,
                           void* stream);
/* srgd_image_backproject for n_images >= 1 images held in flat fp32 buffers.  hw_host = h_0, w_0, h_1, w_1, ... (the LR sizes); image
 * i's planes [3][4h_i][4w_i] begin at element offsets_host[i] >= 0 of out01, cond01 and dst01 alike (the layout
 * srgd_image_color_fix_images takes); its scratch follows the scratch of image i-1.  dst01 == out01 is allowed and means in place;
 * any other overlap of the elements dst01 covers with those out01 or cond01 cover is an error.
 * One launch sequence (2 + 2 N launches) covers up to 128 images (the grid's y index is the image, its record travels as a kernel
 * argument; a larger group runs as consecutive sequences of 128).  Every byte of an image is bit-identical to srgd_image_backproject
 * on that image alone, in any group and at any offsets.  Every image is checked before the first launch: on an error nothing is
 * written.
 * scratch: sum_i 2 * roundup(48*h_i*w_i, 256) + roundup(3*h_i*w_i, 256) bytes. */
int srgd_image_backproject_images(const float* out01, const float* cond01, const int64_t* offsets_host, const int32_t* hw_host,
                                  int n_images, int iterations, float* dst01, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
