/* C ABI of libsrgd_metrics.so: quality numbers of super-resolved images on the MI355X (gfx950).  Engine-free: raw device pointers and
 * sizes, no engine handle, no torch types.  A library of its own beside libsrgd_hip.so (include/srgd_hip.h), built by the same
 * srgd_amd/build.py from srgd_amd/csrc/metrics.hip: evaluation is no part of the sampling engine's export table. */
#ifndef SRGD_METRICS_H
#define SRGD_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_image_metrics_last_error(void);

/* Quality numbers of a sampler output against its ground truth (engine extension, absent upstream): Y-channel PSNR, RGB PSNR and
 * Y-channel SSIM with a border crop, the protocol of the x4 super-resolution literature.  out01: device fp32 planar [3][h][w], the
 * [0,1] output of srgd_sampler_end (after srgd_image_color_fix of srgd_hip.h where one ran); ref_u8: device uint8 [h][w][3], the ground truth as
 * decoded; crop >= 0: both lose `crop` pixels on every side first (ch = h - 2*crop, cw = w - 2*crop).
 *   quantisation: q = (int)(out01 * 255.0f) - the fp32 product and truncation of srgd_image_unit_to_u8, so the numbers describe the
 *     image as saved; all further arithmetic is float64 without contraction.
 *   luma: Y = 65.481*(R/255) + 128.553*(G/255) + 24.966*(B/255) + 16 (BT.601 as MATLAB's rgb2ycbcr), not rounded.
 *   psnr_y = 10*log10(255^2 / mean((Yo - Yr)^2)); psnr_rgb the same over the three quantised channels; a mean of exactly 0: +inf.
 *   ssim_y: 11x11 Gaussian window, sigma 1.5 (weights exp(-(i-5)^2/4.5) normalised to sum 1, applied separably), over the
 *     (ch-10) x (cw-10) valid positions; C1 = (0.01*255)^2, C2 = (0.03*255)^2; per position
 *     ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)), s.. = filtered product - product of means; the mean of the map.
 * results: device double [4] = psnr_y, psnr_rgb, ssim_y, n_nonfinite.  A non-finite out01 value inside the cropped region makes the
 * three numbers of that image NaN (n_nonfinite counts them); one in the cropped-off border is not read.
 * ch < 11 or cw < 11 (no SSIM position) is an error: -1, nothing is launched; the message: srgd_image_metrics_last_error().  An image has at most 2^31 - 256 elements (3*h*w).
 * scratch: device memory owned by the caller, 8-byte aligned, of 32 * ceil((h - 2*crop - 10) / 8) * ceil((w - 2*crop - 10) / 32)
 *   bytes: one record of four doubles per 32x8 tile of SSIM positions, summed without atomics in an order that (h, w, crop) fix.
 * Two launches.  Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_image_metrics(const float* out01, const uint8_t* ref_u8, int h, int w, int crop, double* results, double* scratch,
                       void* stream);
/* srgd_image_metrics for n_images images held in flat buffers (the layout of a mixed lock-step run): image i's [3][h_i][w_i] planes
 * start at element out_offsets_host[i] of out01, its [h_i][w_i][3] bytes at byte ref_offsets_host[i] of ref_u8; hw_host = h_0, w_0,
 * h_1, w_1, ...; results: device double [n_images][4].  Offsets need no alignment.  One launch sequence (two launches) covers up to
 * 128 images (the grid's y index is the image; a larger group runs as consecutive sequences of 128).  Each image's four doubles are
 * bit-identical to srgd_image_metrics on that image alone.  Every image is checked before the first launch: on an error nothing is
 * written.  n_images = 0 does nothing and returns 0.
 * scratch: sum_i 32 * ceil((h_i - 2*crop - 10) / 8) * ceil((w_i - 2*crop - 10) / 32) bytes. */
int srgd_image_metrics_images(const float* out01, const uint8_t* ref_u8, const int64_t* out_offsets_host,
                              const int64_t* ref_offsets_host, const int32_t* hw_host, int n_images, int crop, double* results,
                              double* scratch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
