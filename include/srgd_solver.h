/* C ABI of libsrgd_solver.so: the history step of the second-order multistep solver (DPM-Solver++ 2M) of the tiled DDPM sampler on
 * the MI355X (gfx950) - after a sampling step, the difference between the step's prediction of the clean image (x_start) and the
 * previous step's (x_prev) is added to the image canvas with the step's history weight, and the prediction becomes the history.
 * Engine-free: raw device pointers and a host record array; no engine handle, no torch types.  A library of its own beside
 * libsrgd_hip.so (include/srgd_hip.h), libsrgd_metrics.so, libsrgd_ensemble.so, libsrgd_consistency.so, libsrgd_backproject.so and
 * libsrgd_guidance.so, built by the same srgd_amd/build.py from srgd_amd/csrc/solver.hip: none of their export tables changes. */
#ifndef SRGD_SOLVER_H
#define SRGD_SOLVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One image of a call: its [3][Hp][Wp] fp32 canvas begins at element canvas_off of img, of x_start and of x_prev alike.  The box is
 * rows top .. top + h, columns left .. left + w of every canvas plane: the inner box of the image's odd tile grid, the part of the
 * canvas that is never re-noised and so has a history. */
typedef struct srgd_solver_image {
  int64_t canvas_off;
  int32_t Hp, Wp, top, left, h, w;
} srgd_solver_image;

/* Message of the calling thread's last failed call (valid until its next call). */
const char* srgd_solver_last_error(void);

/* One history step on n >= 1 images (engine extension, absent upstream).  Per element inside each image's box, fp32, every
 * operation rounded on its own (no fused multiply-add), so that numpy fp32 reproduces it bit for bit:
 *   d = x_start - x_prev;  if (w != 0) img = img + w * d;  x_prev = x_start.
 * With w == 0 img is neither read nor written: it keeps its bytes even where x_prev is NaN.  Everything outside the boxes keeps its
 * bytes in all three buffers.  There are no clamps: an element where x_start is NaN or Inf comes out non-finite in img (w != 0) and in
 * x_prev, and no other element sees it.
 * With the update A * x_t + B * x0 of a deterministic step, w = B / (2 r), r = h_prev / h the ratio of the two steps' half log-SNR
 * widths, makes the step the 2M one: x0 + (x0 - x0_prev) / (2 r) in place of x0.
 * Work split.  One launch per call and per 128 images, workgroups of 256 threads over 8 rows of a box; the grid's y index is the
 * image, its z index the plane; the records travel as a kernel argument.  Rows are read and written dword by dword along the row, or
 * four dwords at a time where the box's first element, the canvas row and the plane are multiples of four elements and the three
 * pointers are 16-byte aligned; both forms give the same bytes.  No atomics: every element depends on itself alone, so every image
 * comes out bit-identical to the call on that image alone, in any group and at any offsets.
 * Layout.  img, x_start and x_prev are 4-byte aligned.  The canvases of a call are pairwise disjoint; the elements the call covers in
 * img, x_start and x_prev do not overlap each other.  3*Hp*Wp < 2^31.
 * Errors (-1, nothing is launched, nothing is written; the message: srgd_solver_last_error()): a null pointer, n < 1, h or w < 1, a
 * box that leaves its canvas, a negative offset, 3*Hp*Wp >= 2^31, a w that is NaN or Inf, a misaligned pointer, overlapping canvases
 * or buffers.  Every image is checked before the first launch.
 * Asynchronous on `stream`; no allocation, no synchronisation. */
int srgd_solver_history_step(float* img, const float* x_start, float* x_prev, const srgd_solver_image* recs, int n, float w,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif
