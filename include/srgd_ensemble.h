/* C ABI of libsrgd_ensemble.so: the mean image and the spread map of the K samples of an image on the MI355X (gfx950).  Engine-free:
 * raw device pointers and sizes, no engine handle, no torch types.  A library of its own beside libsrgd_hip.so (include/srgd_hip.h)
 * and libsrgd_metrics.so (include/srgd_metrics.h), built by the same srgd_amd/build.py from srgd_amd/csrc/ensemble.hip: neither of
 * their export tables changes. */
#ifndef SRGD_ENSEMBLE_H
#define SRGD_ENSEMBLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_image_ensemble_last_error(void);

/* Mean image and spread map of the K samples of one image (engine extension, absent upstream).  Every input is a uint8 sample AS
 * SAVED, so every output but one averaged scalar is an exact function of integers.
 * Definition.  K samples, each uint8 [h][w][3], 2 <= K <= 256.  For every one of the 3*h*w elements, with x_k its K values:
 *   S = sum x_k,  Q = sum x_k^2,  D = K*Q - S^2   (D >= 0; 64-bit integer arithmetic)
 *   mean image, uint8 [h][w][3]:  m = (2*S + K) div (2*K)   (integer division: the nearest integer, halves up)
 *   spread map, uint8 [h][w][3]:  twice the population standard deviation sigma = sqrt(D)/K (sigma <= 127.5, so 2 sigma <= 255),
 *     rounded to the nearest integer with halves up, defined BY INTEGERS: s = 0 if 16*D < K^2, else the one s in 1..255 with
 *     (2s-1)^2 * K^2 <= 16*D < (2s+1)^2 * K^2.  (The kernel estimates s in fp32 and settles it with this comparison.)
 *   mean01 (optional, NULL = not written), fp32 planar [3][h][w]:  (float)m / 255.0f, the mean image as ToTensor reads the PNG back.
 *   stats, two doubles in 8-bit units:  mean_std = (sum_e sqrt((double)D_e) / K) / (3*h*w)  and  max_std = sqrt((double)max_e D_e) / K.
 *     max_std is exact (an integer maximum, one square root, one division).  mean_std is the only sum of floats: the image's
 *     elements are cut into fixed chunks of 4096 consecutive elements, a chunk's square roots are added in a fixed order into one
 *     plainly stored record, and a second kernel, one workgroup per image, adds the records in a fixed order.  No atomics.
 *     Chunks and both orders depend on (h, w) alone.
 * Layout.  Sample k begins at byte k*stride of `samples`, stride = 3*h*w rounded up to a multiple of 16; `samples`, mean_u8 and
 * std_u8 are 16-byte aligned (a lane works on 16 consecutive bytes per sample with 16-byte loads), mean01 4-byte, stats and scratch
 * 8-byte aligned.  The last (3*h*w mod 16) bytes of an image are read and written byte by byte: the padding of a sample is never
 * read, nothing beyond the 3*h*w bytes of mean_u8 / std_u8 and the 3*h*w floats of mean01 is ever written.
 * scratch: device memory owned by the caller, 16 * ceil(3*h*w / 4096) bytes (one record of two 8-byte words per chunk).
 * Errors (-1, nothing is launched, nothing is written; the message: srgd_image_ensemble_last_error()): a null pointer other than
 * mean01, K outside 2..256, h or w < 1, 3*h*w >= 2^31 - 256, a misaligned pointer.
 * Two launches.  Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_image_ensemble(const uint8_t* samples, int n_samples, int h, int w, uint8_t* mean_u8, uint8_t* std_u8, float* mean01,
                        double* stats, double* scratch, void* stream);
/* srgd_image_ensemble for n_images >= 1 images held in flat buffers, n_samples = K shared by the call.  hw_host = h_0, w_0, h_1,
 * w_1, ...; sample k of image i begins at byte sample_offsets_host[i] + k*stride_i of `samples`, stride_i = 3*h_i*w_i rounded up to a
 * multiple of 16; image i's mean and spread begin at byte out_offsets_host[i] of mean_u8 and of std_u8; its three mean01 planes at
 * element mean01_offsets_host[i] of mean01 (mean01 and mean01_offsets_host are NULL together); stats: device double [n_images][2] =
 * mean_std, max_std.  Sample and output offsets are multiples of 16 in [0, 2^36) - anything else is an error before any launch;
 * mean01 offsets are >= 0 and need no alignment.
 * One launch sequence (two launches) covers up to 128 images (the grid's y index is the image, its record travels as a kernel
 * argument; a larger group runs as consecutive sequences of 128).  Every byte and both doubles of an image are bit-identical to
 * srgd_image_ensemble on that image alone, in any group and at any offsets.  Every image is checked before the first launch: on an
 * error nothing is written.
 * scratch: sum_i 16 * ceil(3*h_i*w_i / 4096) bytes. */
int srgd_image_ensemble_images(const uint8_t* samples, const int64_t* sample_offsets_host, const int32_t* hw_host, int n_images,
                               int n_samples, uint8_t* mean_u8, uint8_t* std_u8, const int64_t* out_offsets_host, float* mean01,
                               const int64_t* mean01_offsets_host, double* stats, double* scratch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
