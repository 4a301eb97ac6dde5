// Pillow-exact resize of 8-bit RGB images by any ratio up to 8 either way on the GPU (engine extension, absent upstream): what
// PIL.Image.resize((w_out, h_out), BICUBIC | BILINEAR | LANCZOS) gives, bit for bit.  The definition is fixed in
// include/srgd_resize.h and restated here in short: per axis a table of clipped, renormalised windows in 22-bit fixed point
// (computed on the host in double, in Pillow's order), the horizontal pass over all input rows rounded to 8 bits, then the vertical
// pass on that result; a pass whose in == out is skipped.
//
// The two passes, their work split and the host driver are pillow_resample.hpp's (shared with alpha.hip, as a header); here they
// are instantiated for 3 channels, a horizontal tile of 32 output pixels x 16 rows and two rows per thread (rows r and r + 8: a
// coefficient serves six products), and image bases that are only known to be what the caller gave: rows of 3 w bytes with
// w % 4 != 0, or on a base that is not dword aligned, take the guarded byte path of each kernel.
// LDS: horizontal 14,656 (rows) + 6,272 (coefficients) + 256 (bounds) + 1,536 (result) = 22,720 bytes; vertical 3,136 + 128.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_resize.h"
#include "pillow_resample.hpp"

// This file is a library of its own (libsrgd_resize.so, include/srgd_resize.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing, pillow_resample.hpp the resize it has in common with alpha.hip.
namespace srgd {
namespace {

constexpr int RS_HW = 32, RS_R = 2;                  // horizontal tile: 32 output pixels x 16 rows, two rows per thread
static_assert(PR_MAX_SIDE == SRGD_RESIZE_MAX_SIDE && PR_MAX_RATIO == SRGD_RESIZE_MAX_RATIO && PR_MAX_TAPS == SRGD_RESIZE_MAX_TAPS,
              "the limits of include/srgd_resize.h");
static_assert(SRGD_RESIZE_LANCZOS == pillow::LANCZOS && SRGD_RESIZE_BILINEAR == pillow::BILINEAR && SRGD_RESIZE_BICUBIC == pillow::BICUBIC,
              "the filters of pillow_coeffs.hpp");

__global__ __launch_bounds__(PR_THREADS) void resize_horizontal_kernel(PrTable tab, const unsigned char* __restrict__ src,
                                                                       unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                       const unsigned char* __restrict__ tables) {
  pr_horizontal<3, RS_HW, RS_R, false>(tab, src, scratch, dst, tables);
}

__global__ __launch_bounds__(PR_THREADS) void resize_vertical_kernel(PrTable tab, const unsigned char* __restrict__ src,
                                                                     const unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                     const unsigned char* __restrict__ tables) {
  pr_vertical<3, false>(tab, src, scratch, dst, tables);
}

// ------------------------------------------------------------------------------------------------ host (Pillow's tables: pillow_coeffs.hpp)
int resize_images(const void* src, void* dst, const srgd_resize_image* images, int n_images, int filter, const void* tables,
                  long long tables_bytes, void* scratch, long long scratch_bytes, hipStream_t st) {
  const std::string name("srgd_resize_u8_images");
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!src || !dst || !images || !tables || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (pillow::filter_support(filter) == 0.0) SRGD_EXT_FAIL(name + ": unknown filter (1 lanczos, 2 bilinear, 3 bicubic)");
  const auto ksize_of = [filter](const srgd_resize_image& im, bool h) {
    return h ? pillow::ksize(im.w_in, im.w_out, filter) : pillow::ksize(im.h_in, im.h_out, filter);
  };
  return pr_resize<3, RS_HW, false>(name, "images", src, dst, images, n_images, ksize_of, tables, tables_bytes, scratch, scratch_bytes,
                                    resize_horizontal_kernel, resize_vertical_kernel, st);
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_resize_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_resize_ksize(int in_size, int out_size, int filter) {
  if (pillow::filter_support(filter) == 0.0) SRGD_EXT_FAIL("srgd_resize_ksize: unknown filter (1 lanczos, 2 bilinear, 3 bicubic)");
  if (const char* problem = axis_problem(in_size, out_size)) SRGD_EXT_FAIL(std::string("srgd_resize_ksize: ") + problem);
  return pillow::ksize(in_size, out_size, filter);
}

SRGD_EXT_EXPORT int srgd_resize_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coeffs) {
  if (!bounds || !coeffs) SRGD_EXT_FAIL("srgd_resize_coeffs: null argument");
  if (pillow::filter_support(filter) == 0.0) SRGD_EXT_FAIL("srgd_resize_coeffs: unknown filter (1 lanczos, 2 bilinear, 3 bicubic)");
  if (const char* problem = axis_problem(in_size, out_size)) SRGD_EXT_FAIL(std::string("srgd_resize_coeffs: ") + problem);
  pillow::axis_table(in_size, out_size, filter, bounds, coeffs);
  return 0;
}

SRGD_EXT_EXPORT int srgd_resize_u8_images(const void* src, void* dst, const srgd_resize_image* images_host, int n_images, int filter,
                                          const void* tables, int64_t tables_bytes, void* scratch, int64_t scratch_bytes, void* stream) {
  return resize_images(src, dst, images_host, n_images, filter, tables, (long long)tables_bytes, scratch, (long long)scratch_bytes,
                       (hipStream_t)stream);
}

}  // extern "C"
