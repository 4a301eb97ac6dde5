// The history step of the second-order multistep solver (DPM-Solver++ 2M) of the tiled DDPM sampler on the GPU (engine extension,
// absent upstream): after a sampling step, inside every image's inner box,
//   d = x_start - x_prev;  if (w != 0) img = img + w * d;  x_prev = x_start
// in fp32 with every operation rounded on its own; the definition is fixed in include/srgd_solver.h and restated here in short.
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument), blockIdx.z the plane, blockIdx.x a band of 8 rows
// of the box; the 256 threads of a workgroup walk the band's rows unit by unit, consecutive threads on consecutive units of a row.  A
// unit is one dword, or four (one 16-byte access per buffer and lane, a wave covers 1 KiB of a row) where the host found that every
// row of the box begins on a 16-byte boundary in all three buffers; the last unit of a row whose width is no multiple of four is
// finished dword by dword.  Both forms do the same three operations per element, so they give the same bytes.
// No LDS, no atomics, no reductions: every element depends on itself alone - bit-identical alone, in any group, at any offset.
// Bytes moved per element: 8 read (x_start, x_prev) + 4 written (x_prev), and 4 + 4 more (img) when w != 0.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_solver.h"
#include "ext_common.hpp"

// This file is a library of its own (libsrgd_solver.so, include/srgd_solver.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing (pillow_resample.hpp and pillow_x4.hpp, the code some of them have in
// common, are headers too: no symbol is shared).
namespace srgd {
namespace {

constexpr int SV_THREADS = 256;
constexpr int SV_ROWS = 8;                           // rows of a box per workgroup
constexpr int SV_MAX_IMAGES = 128;                   // records travel as a kernel argument (4 KiB)

typedef float sv_f32x4 __attribute__((ext_vector_type(4)));

struct SvImage {
  long long base;                                    // element of the box's first pixel in plane 0 of the three buffers
  int plane, Wp;                                     // Hp * Wp; the canvas row
  int h, w;                                          // the box
  int vec, pad;                                      // 1: every row of the box begins on a 16-byte boundary in all three buffers
};
struct SvTable { SvImage im[SV_MAX_IMAGES]; };

__device__ __forceinline__ void sv_element(float* __restrict__ img, const float* __restrict__ xs, float* __restrict__ xp, long long o,
                                           float w) {
#pragma clang fp contract(off)
  const float s = xs[o];
  const float d = s - xp[o];
  if (w != 0.0f) img[o] = img[o] + w * d;
  xp[o] = s;
}

__global__ __launch_bounds__(SV_THREADS) void solver_history_kernel(SvTable tab, float* __restrict__ img,
                                                                    const float* __restrict__ x_start, float* __restrict__ x_prev,
                                                                    float w) {
#pragma clang fp contract(off)
  const SvImage im = tab.im[blockIdx.y];
  const int y0 = (int)blockIdx.x * SV_ROWS;
  if (y0 >= im.h) return;                                            // the grid is as tall as the launch's tallest box
  const int rows = min(SV_ROWS, im.h - y0);
  const long long origin = im.base + (long long)blockIdx.z * im.plane + (long long)y0 * im.Wp;   // < canvas_off + 3 * Hp * Wp
  if (im.vec) {
    const int units = (im.w + 3) >> 2;
    for (int i = (int)threadIdx.x; i < rows * units; i += SV_THREADS) {
      const int r = i / units, u = i - r * units;
      const long long o = origin + (long long)r * im.Wp + 4 * u;
      if (4 * u + 4 <= im.w) {
        const sv_f32x4 s = *reinterpret_cast<const sv_f32x4*>(x_start + o);
        const sv_f32x4 d = s - *reinterpret_cast<const sv_f32x4*>(x_prev + o);
        if (w != 0.0f) {
          sv_f32x4* pi = reinterpret_cast<sv_f32x4*>(img + o);
          *pi = *pi + w * d;
        }
        *reinterpret_cast<sv_f32x4*>(x_prev + o) = s;
      } else {
        for (int x = 4 * u; x < im.w; ++x) sv_element(img, x_start, x_prev, o + (x - 4 * u), w);
      }
    }
  } else {
    for (int i = (int)threadIdx.x; i < rows * im.w; i += SV_THREADS) {
      const int r = i / im.w, x = i - r * im.w;
      sv_element(img, x_start, x_prev, origin + (long long)r * im.Wp + x, w);
    }
  }
}

int history_step(float* img, const float* x_start, float* x_prev, const srgd_solver_image* recs, int n, float w, hipStream_t st) {
  const std::string name("srgd_solver_history_step");
  if (n < 1) SRGD_EXT_FAIL(name + ": n must be >= 1");
  if (!img || !x_start || !x_prev || !recs) SRGD_EXT_FAIL(name + ": null argument");
  if (!std::isfinite(w)) SRGD_EXT_FAIL(name + ": w must be finite");
  if ((((uintptr_t)img | (uintptr_t)x_start | (uintptr_t)x_prev) & 3u) != 0) SRGD_EXT_FAIL(name + ": img, x_start and x_prev must be 4-byte aligned");
  long long lo = 0, hi = 0;                              // the elements the call covers in the three buffers
  for (int i = 0; i < n; ++i) {                          // every image is checked before the first launch
    const srgd_solver_image& m = recs[i];
    if (m.h < 1 || m.w < 1) SRGD_EXT_FAIL(name + ": bad size (h and w must be >= 1)");
    if (m.Hp < 1 || m.Wp < 1 || (long long)m.Hp * m.Wp > ((1ll << 31) - 1) / 3) SRGD_EXT_FAIL(name + ": bad canvas (3*Hp*Wp must be in 1 .. 2^31 - 1)");
    if (m.top < 0 || m.left < 0 || (long long)m.top + m.h > m.Hp || (long long)m.left + m.w > m.Wp) SRGD_EXT_FAIL(name + ": the box leaves its canvas");
    if (m.canvas_off < 0 || m.canvas_off >= (1ll << 40)) SRGD_EXT_FAIL(name + ": offset outside [0, 2^40)");
    const long long canvas = 3ll * m.Hp * m.Wp;
    lo = i == 0 ? m.canvas_off : std::min<long long>(lo, m.canvas_off);
    hi = i == 0 ? m.canvas_off + canvas : std::max<long long>(hi, m.canvas_off + canvas);
  }
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const Range a{recs[i].canvas_off, recs[i].canvas_off + 3ll * recs[i].Hp * recs[i].Wp};
      const Range b{recs[j].canvas_off, recs[j].canvas_off + 3ll * recs[j].Hp * recs[j].Wp};
      if (a.meets(b)) SRGD_EXT_FAIL(name + ": overlapping canvases");
    }
  const Range r_img{(long long)(intptr_t)img + 4 * lo, (long long)(intptr_t)img + 4 * hi};
  const Range r_xs{(long long)(intptr_t)x_start + 4 * lo, (long long)(intptr_t)x_start + 4 * hi};
  const Range r_xp{(long long)(intptr_t)x_prev + 4 * lo, (long long)(intptr_t)x_prev + 4 * hi};
  if (r_img.meets(r_xs) || r_img.meets(r_xp) || r_xs.meets(r_xp)) SRGD_EXT_FAIL(name + ": overlapping buffers (img, x_start and x_prev are disjoint)");
  const bool aligned16 = (((uintptr_t)img | (uintptr_t)x_start | (uintptr_t)x_prev) & 15u) == 0;
  for (int first = 0; first < n; first += SV_MAX_IMAGES) {            // one launch per SV_MAX_IMAGES images
    const int cnt = std::min(SV_MAX_IMAGES, n - first);
    SvTable tab;
    int max_h = 0;
    for (int k = 0; k < SV_MAX_IMAGES; ++k) tab.im[k] = SvImage{0ll, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < cnt; ++k) {
      const srgd_solver_image& m = recs[first + k];
      const long long base = m.canvas_off + (long long)m.top * m.Wp + m.left;
      const long long plane = (long long)m.Hp * m.Wp;
      const int vec = aligned16 && base % 4 == 0 && m.Wp % 4 == 0 && plane % 4 == 0 ? 1 : 0;
      tab.im[k] = SvImage{base, (int)plane, m.Wp, m.h, m.w, vec, 0};
      max_h = std::max(max_h, m.h);
    }
    const dim3 grid((unsigned)((max_h + SV_ROWS - 1) / SV_ROWS), (unsigned)cnt, 3u);
    hipLaunchKernelGGL(solver_history_kernel, grid, dim3(SV_THREADS), 0, st, tab, img, x_start, x_prev, w);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_solver_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_solver_history_step(float* img, const float* x_start, float* x_prev, const srgd_solver_image* recs, int n, float w,
                                             void* stream) {
  return history_step(img, x_start, x_prev, recs, n, w, (hipStream_t)stream);
}

}  // extern "C"
