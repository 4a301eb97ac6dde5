/* C ABI of libsrgd_threshold.so: dynamic thresholding (Imagen's percentile clipping) of the tiled DDPM sampler's prediction of the
 * clean image on the MI355X (gfx950) - after a sampling step taken without the static clamp (srgd_step_scalars.no_clamp of
 * include/srgd_hip.h), every image's x_start is clipped to [-s, s] and divided by s, s >= 1 an exact quantile of |x_start| inside the
 * image's crop box, and the image canvas receives the same correction scaled by the posterior mean's weight of x_start.
 * Engine-free: raw device pointers, a host record array and a caller-owned scratch; no engine handle, no torch types.  A library of
 * its own beside libsrgd_hip.so and the eight other extension libraries, built by the same srgd_amd/build.py from
 * srgd_amd/csrc/threshold.hip (with -ffp-contract=off): none of their export tables changes. */
#ifndef SRGD_THRESHOLD_H
#define SRGD_THRESHOLD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One image of a call: its [3][Hp][Wp] fp32 canvas begins at element canvas_off of img and of x_start alike.
 * The statistics box - rows top .. top + H, columns left .. left + W of every plane: the crop box - is where the quantile is taken.
 * The update box - rows box_t .. box_t + box_h, columns box_l .. box_l + box_w - is where x_start and img are rewritten: what the
 * step wrote (the whole canvas on even steps, the inner box on odd steps).  The statistics box lies inside the update box. */
typedef struct srgd_threshold_image {
  int64_t canvas_off;
  int32_t Hp, Wp;
  int32_t top, left, H, W;
  int32_t box_t, box_l, box_h, box_w;
} srgd_threshold_image;

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_threshold_last_error(void);

/* The position of quantile q among n sorted values (host only, no GPU):
 *   pos = (double)q * (double)(n - 1);  lo = floor(pos);  hi = min(lo + 1, n - 1);  frac = (float)(pos - lo).
 * Returns 0, or -1 for NULL, n < 1, or q outside (0, 1] / NaN. */
int srgd_threshold_position(int64_t n, float q, int64_t* lo, int64_t* hi, float* frac);

/* Bytes of the scratch a call on n_images images needs (host only): 8448 per image (a histogram of 2048 counters and the state of
 * the selection).  0 for n_images < 1. */
uint64_t srgd_threshold_scratch_bytes(int n_images);

/* Elements of the statistics box one workgroup of the histogram kernels counts (host only): the sizes around which a test places
 * its cases. */
int srgd_threshold_chunk_elems(void);

/* One thresholding step on n_images >= 1 images (engine extension, absent upstream).  Per image:
 * Keys.  key(v) is the bit pattern of v with the sign bit cleared, compared as uint32: +0 and -0 are equal, denormals are ordered,
 *   +Inf is below every NaN, NaNs sort last.  a_0 <= .. <= a_{N-1} are the N = 3*H*W keys of the statistics box of x_start, sorted.
 * Position.  (lo, hi, frac) = srgd_threshold_position(N, q).
 * Threshold.  s_raw = a_lo + frac * (a_hi - a_lo), the keys read as fp32, in fp32 with a separate subtraction, multiplication and
 *   addition (no fused multiply-add); s = (s_raw < 1) ? 1 : s_raw, so a NaN s_raw stays NaN.  s is written to s_out[i].
 * Apply, to every element v of the update box of x_start, all three planes (the comparisons are false for a NaN v or a NaN s):
 *   t = v < -s ? -s : (v > s ? s : v);  y = t / s (IEEE division);  d = y - v;  x_start = y;
 *   if d != 0: img = img + weight_img * d (a separate multiplication and addition); otherwise the element of img is not written.
 * A non-finite s has no special case: a NaN s makes the whole update box NaN in both canvases, so a non-finite result stays visible.
 * A NaN v comes out NaN in both canvases.  Everything outside the update boxes keeps its bytes.  With s = 1 the result is the static
 * clamp, and img keeps its bytes wherever |v| <= 1.
 * With the DDPM posterior mean alpha_next * (x_t * (1 - c) / alpha + c * x0), linear in x0, weight_img = alpha_next * c applies to the
 * canvas the change of x0.
 * Work split.  Per call one clear of the scratch; per 128 images three histogram passes over the statistics box - a radix select on
 * the 31-bit keys with digits of 11, 10 and 10 bits - each followed by a one-workgroup-per-image scan, and one apply kernel.  The
 * selection carries two states (prefix, remaining rank) per image, for lo and for hi; they may part ways at any digit, and a pass
 * counts the keys under either prefix.  A workgroup counts 4096 keys in LDS (a wave first folds the lanes that share a counter:
 * |x_start| concentrates in a few exponent bins) and adds its non-empty counters to the image's with one unsigned integer atomic
 * each.  Integer sums do not depend on their order: s is bit-reproducible, and an image of a group comes out bit-identical to the
 * call on that image alone, in any group and at any offsets.  After the third scan the prefixes are a_lo and a_hi.  The grid's y
 * index is the image; the records travel as kernel arguments.  No floating-point atomics anywhere.
 * Layout.  img, x_start and s_out are 4-byte aligned, scratch is 256-byte aligned.  The canvases of a call are pairwise disjoint; the
 * elements the call covers in img, x_start, s_out and the scratch do not overlap each other.  3*Hp*Wp < 2^31.
 * scratch: device memory owned by the caller, srgd_threshold_scratch_bytes(n_images) bytes; its contents before and after are of no
 * interest.
 * Errors (-1, nothing is launched, nothing is written; the message: srgd_threshold_last_error()): a null pointer, n_images < 1, q
 * outside (0, 1] or NaN, a weight_img that is NaN or Inf, H or W < 1, a statistics box not inside the update box, an update box not
 * inside the canvas, a negative offset, 3*Hp*Wp >= 2^31, a misaligned pointer, overlapping canvases or buffers.  Every image is
 * checked before the first launch.
 * Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_threshold_step(float* img, float* x_start, const srgd_threshold_image* images_host, int n_images, float q, float weight_img,
                        float* s_out, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
