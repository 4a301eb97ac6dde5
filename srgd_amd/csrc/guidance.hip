// LR-consistency guidance of the tiled DDPM sampler on the GPU (engine extension, absent upstream): after a sampling step the model's
// prediction of the clean image is pulled towards the low-resolution input, g = C - U(D(x_start)), x_start += weight_x0 * g,
// img += weight_img * g inside every image's crop box.  D and U are the x4 reduction and enlargement of Pillow's bicubic with the
// project's 22-bit coefficient integers divided by 2^22, in fp32 with no rounding to 8 bits and no clipping anywhere; the definition
// is fixed in include/srgd_guidance.h and restated here in short.
//
// The window facts are those of backproject.hip.  Reduction (4n -> n, n >= 5): output i in 2 .. n-3 reads the 16 inputs from 4i - 6
// with one symmetric vector; outputs 0, 1, n-2, n-1 read 10, 14, 14, 10 inputs of the clipped window with vectors of their own.
// Enlargement (n -> 4n): output j in 6 .. 4n-7 reads the 4 inputs from (j - 6) / 4 with the vector of its phase (j - 6) % 4; outputs
// 0 .. 5 and 4n-6 .. 4n-1 read 2 or 3 inputs with vectors of their own.  Every vector is laid on the frame of its output -
// [4i - 6, 4i + 10) for the reduction, [floor((j - 6) / 4), + 4) for the enlargement - with zeros on the taps outside the image, and
// the inputs outside the image are staged as zeros: a zero tap never meets an element of the image, so a NaN spreads exactly as far
// as Pillow's windows reach.
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument), blockIdx.z the plane.
//   reduce: one workgroup of 256 threads per tile of 32 x 15 LR pixels.  The HR patch of the tile - 72 rows from 4 ty0 - 6, 144
//           columns from 4 tx0 - 8 (a halo of 8, of which the windows use 6) - goes from x_start to LDS, zeros outside the crop box;
//           horizontal pass LDS to LDS (a thread owns one LR column, its 16 coefficients stay in registers, and takes every 8th
//           row); vertical pass; D stored to the scratch.
//   update: one workgroup per tile of 128 x 60 HR pixels = the same 32 x 15 LR pixels.  The tile's D rows and columns plus a halo
//           of 2 (19 x 36, zeros outside the image) go to LDS; horizontal pass to 19 rows x 128 in LDS (a thread owns one HR
//           column and takes every second row); vertical pass and the update: a thread takes one element of an HR row, reads the
//           condition, x_start and img at that element and writes the two canvases there - a workgroup reads the canvases only at
//           the elements it writes.
// No atomics, no reductions across workgroups: every element depends on its own image's elements alone - bit-identical alone, in
// any group, at any offset.  LDS: reduce 41,472 (patch) + 9,216 (h-pass) + 320 = 51,008 bytes; update 2,736 + 9,728 + 256 = 12,720.
// Bytes moved per call and HR pixel of a plane: reduce reads 4 * 1.35 (the patch with its halo) and writes 0.25; update reads
// 12 (condition, x_start, img) + 0.36 (D) and writes 8.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_guidance.h"
#include "pillow_x4.hpp"

// This file is a library of its own (libsrgd_guidance.so, include/srgd_guidance.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing, pillow_x4.hpp the selectors of the x4 vectors it has in common with
// consistency.hip and backproject.hip.
namespace srgd {
namespace {

constexpr int GD_THREADS = 256;
constexpr int GD_TW = 32, GD_TH = 15;                // LR pixels of a tile
constexpr int GD_MAX_IMAGES = 128;                   // records travel as a kernel argument (5 KiB)
// reduce
constexpr int GD_RTAPS = 16;
constexpr int GD_PROWS = 4 * GD_TH + 12;             // HR rows of the patch: 72 (rows 4 ty0 - 6 .. 4 ty0 + 65)
constexpr int GD_PCOLS = 4 * GD_TW + 16;             // HR columns of the patch: 144 (columns 4 tx0 - 8 .. 4 tx0 + 135)
static_assert(GD_PROWS % (GD_THREADS / GD_TW) == 0, "the h-pass gives every thread the same number of rows");
static_assert(4 * (GD_TW - 1) + 2 + GD_RTAPS <= GD_PCOLS, "the window of the last column lies inside the patch row");
static_assert(4 * (GD_TH - 1) + GD_RTAPS <= GD_PROWS, "the window of the last row lies inside the patch");
// update
constexpr int GD_UTAPS = 4;
constexpr int GD_UW = 4 * GD_TW, GD_UH = 4 * GD_TH;  // HR pixels of a tile: 128 x 60
constexpr int GD_DROWS = GD_TH + 4;                  // LR rows of the D patch: 19 (rows ty0 - 2 .. ty0 + 16)
constexpr int GD_DCOLS = GD_TW + 4;                  // LR columns of the D patch: 36 (columns tx0 - 2 .. tx0 + 33)
static_assert(GD_THREADS == 2 * GD_UW, "the enlargement's h-pass: a thread per HR column, two rows at a time");
static_assert(((GD_UW - 1 + 2) >> 2) + GD_UTAPS <= GD_DCOLS, "the 4 columns of the last HR column lie inside the D patch row");
static_assert(((GD_UH - 1 + 2) >> 2) + GD_UTAPS <= GD_DROWS, "the 4 rows of the last HR row lie inside the D patch");

struct GdImage {
  long long base;                                    // element of the crop box's first pixel in plane 0 of img and x_start
  long long cond;                                    // first element of the image's planes in cond01
  unsigned long long scr;                            // first float of the image's D in the scratch (a multiple of 64)
  int plane, Wp;                                     // Hp * Wp; the canvas row
  int h, w;                                          // LR size
};
struct GdTable { GdImage im[GD_MAX_IMAGES]; };
struct GdDown { float k[5][GD_RTAPS]; };             // row 0, row 1, interior, row n-2, row n-1, each on the frame [4i - 6, 4i + 10)
struct GdUp { float k[16][GD_UTAPS]; };              // indices 0 .. 5, phases 0 .. 3, indices 4n-6 .. 4n-1, each on the frame of its output

__host__ __device__ inline unsigned gd_tiles_x(int w) { return (unsigned)((w + GD_TW - 1) / GD_TW); }
__host__ __device__ inline unsigned gd_tiles_y(int h) { return (unsigned)((h + GD_TH - 1) / GD_TH); }
inline unsigned long long gd_scratch(long long h, long long w) { return round_up((unsigned long long)(12 * h * w), 256ull); }

// D = x4 reduction of x_start inside the crop box, fp32.
__global__ __launch_bounds__(GD_THREADS) void guidance_reduce_kernel(GdTable tab, GdDown coeffs, const float* __restrict__ x_start,
                                                                     float* __restrict__ scratch) {
  __shared__ float patch[GD_PROWS * GD_PCOLS];
  __shared__ float hbuf[GD_PROWS * GD_TW];
  __shared__ float kk[5][GD_RTAPS];
  const GdImage im = tab.im[blockIdx.y];
  const int h = im.h, w = im.w, c = (int)blockIdx.z;
  const unsigned tiles_x = gd_tiles_x(w);
  if (blockIdx.x >= tiles_x * gd_tiles_y(h)) return;                 // the grid is as wide as the launch's largest image
  const int tx0 = (int)(blockIdx.x % tiles_x) * GD_TW, ty0 = (int)(blockIdx.x / tiles_x) * GD_TH;
  const int tid = (int)threadIdx.x;
  if (tid < 5 * GD_RTAPS) kk[tid >> 4][tid & 15] = coeffs.k[tid >> 4][tid & 15];

  // 1. the HR patch: patch row r is crop-box row 4 ty0 - 6 + r, patch column q is crop-box column 4 tx0 - 8 + q; zeros outside
  const float* src = x_start + im.base + (long long)c * im.plane;
  for (int i = tid; i < GD_PROWS * GD_PCOLS; i += GD_THREADS) {
    const int r = i / GD_PCOLS, q = i - r * GD_PCOLS;
    const int y = 4 * ty0 - 6 + r, x = 4 * tx0 - 8 + q;
    float val = 0.0f;
    if (y >= 0 && y < 4 * h && x >= 0 && x < 4 * w) val = src[y * im.Wp + x];        // < Hp * Wp < 2^31 / 3
    patch[i] = val;
  }
  __syncthreads();

  // 2. horizontal pass: LR column x of the tile, rows tid / 32 + 8 it.  The frame of output tx0 + x begins at crop-box column
  //    4 (tx0 + x) - 6 = patch column 4 x + 2.
  {
    const int x = tid & (GD_TW - 1);
    float kx[GD_RTAPS];
    const float* kv = kk[x4_down_vector(tx0 + x, w)];
#pragma unroll
    for (int t = 0; t < GD_RTAPS; ++t) kx[t] = kv[t];
    for (int r = tid / GD_TW; r < GD_PROWS; r += GD_THREADS / GD_TW) {
      const float* p = patch + r * GD_PCOLS + 4 * x + 2;
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < GD_RTAPS; ++t) acc = fmaf(kx[t], p[t], acc);
      hbuf[r * GD_TW + x] = acc;
    }
  }
  __syncthreads();

  // 3. vertical pass: LR pixel (yl, x) of the tile; its frame begins at patch row 4 yl
  float* down = scratch + im.scr + (size_t)c * (size_t)h * (size_t)w;
  for (int i = tid; i < GD_TH * GD_TW; i += GD_THREADS) {
    const int yl = i / GD_TW, x = i - yl * GD_TW;
    const int gy = ty0 + yl, gx = tx0 + x;
    if (gy >= h || gx >= w) continue;
    const float* ky = kk[x4_down_vector(gy, h)];
    const float* p = hbuf + 4 * yl * GD_TW + x;
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < GD_RTAPS; ++t) acc = fmaf(ky[t], p[t * GD_TW], acc);
    down[gy * w + gx] = acc;
  }
}

// g = C - U(D);  x_start += weight_x0 * g;  img += weight_img * g, inside the crop box.
__global__ __launch_bounds__(GD_THREADS) void guidance_update_kernel(GdTable tab, GdUp coeffs, float* img, float* x_start,
                                                                     const float* __restrict__ cond01, const float* __restrict__ scratch,
                                                                     float weight_x0, float weight_img) {
  __shared__ float dpatch[GD_DROWS * GD_DCOLS];
  __shared__ float ubuf[GD_DROWS * GD_UW];
  __shared__ float kk[16][GD_UTAPS];
  const GdImage im = tab.im[blockIdx.y];
  const int h = im.h, w = im.w, c = (int)blockIdx.z;
  const unsigned tiles_x = gd_tiles_x(w);
  if (blockIdx.x >= tiles_x * gd_tiles_y(h)) return;
  const int tx0 = (int)(blockIdx.x % tiles_x) * GD_TW, ty0 = (int)(blockIdx.x / tiles_x) * GD_TH;
  const int tid = (int)threadIdx.x;
  if (tid < 16 * GD_UTAPS) kk[tid >> 2][tid & 3] = coeffs.k[tid >> 2][tid & 3];

  // 1. the D patch: patch row r is LR row ty0 - 2 + r, patch column p is LR column tx0 - 2 + p; zeros outside the image
  const float* down = scratch + im.scr + (size_t)c * (size_t)h * (size_t)w;
  for (int i = tid; i < GD_DROWS * GD_DCOLS; i += GD_THREADS) {
    const int r = i / GD_DCOLS, p = i - r * GD_DCOLS;
    const int y = ty0 - 2 + r, x = tx0 - 2 + p;
    float val = 0.0f;
    if (y >= 0 && y < h && x >= 0 && x < w) val = down[y * w + x];
    dpatch[i] = val;
  }
  __syncthreads();

  // 2. horizontal pass: HR column x of the tile, rows tid / 128 + 2 it.  The frame of output 4 tx0 + x begins at LR column
  //    tx0 + floor((x - 6) / 4) = patch column (x + 2) >> 2.
  {
    const int x = tid & (GD_UW - 1);
    const float* kv = kk[x4_up_vector(4 * tx0 + x, 4 * w)];
    const float kx[GD_UTAPS] = {kv[0], kv[1], kv[2], kv[3]};
    for (int r = tid / GD_UW; r < GD_DROWS; r += GD_THREADS / GD_UW) {
      const float* p = dpatch + r * GD_DCOLS + ((x + 2) >> 2);
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < GD_UTAPS; ++t) acc = fmaf(kx[t], p[t], acc);
      ubuf[r * GD_UW + x] = acc;
    }
  }
  __syncthreads();

  // 3. vertical pass and the update: HR pixel (y, x) of the tile; its frame begins at LR row ty0 + floor((y - 6) / 4) = patch row
  //    (y + 2) >> 2
  const long long canvas = im.base + (long long)c * im.plane;
  const float* cnd = cond01 + im.cond + (long long)c * 16 * h * w;
  for (int i = tid; i < GD_UH * GD_UW; i += GD_THREADS) {
    const int y = i / GD_UW, x = i - y * GD_UW;
    const int gy = 4 * ty0 + y, gx = 4 * tx0 + x;
    if (gy >= 4 * h || gx >= 4 * w) continue;
    const float* ky = kk[x4_up_vector(gy, 4 * h)];
    const float* p = ubuf + ((y + 2) >> 2) * GD_UW + x;
    float u = 0.0f;
#pragma unroll
    for (int t = 0; t < GD_UTAPS; ++t) u = fmaf(ky[t], p[t * GD_UW], u);
    const float g = fmaf(2.0f, cnd[gy * (4 * w) + gx], -1.0f) - u;
    const long long o = canvas + gy * im.Wp + gx;
    x_start[o] = fmaf(weight_x0, g, x_start[o]);
    img[o] = fmaf(weight_img, g, img[o]);
  }
}

constexpr float GD_UNIT = 1.0f / (float)(1 << PILLOW_PREC_BITS);   // |k| < 2^23: k * 2^-22 is exact in fp32

// The vectors of pillow_coeffs.hpp on the frames of their outputs, as floats
GdDown framed_down_vectors() {
  int32_t k[5][GD_RTAPS];
  pillow::x4_reduce_vectors(k, true);
  GdDown c;
  for (int v = 0; v < 5; ++v)
    for (int t = 0; t < GD_RTAPS; ++t) c.k[v][t] = (float)k[v][t] * GD_UNIT;
  return c;
}

GdUp framed_up_vectors() {
  int32_t k[16][GD_UTAPS];
  pillow::x4_enlarge_vectors(k, true);
  GdUp c;
  for (int v = 0; v < 16; ++v)
    for (int t = 0; t < GD_UTAPS; ++t) c.k[v][t] = (float)k[v][t] * GD_UNIT;
  return c;
}

int guidance_step(float* img, float* x_start, const float* cond01, const srgd_guidance_image* images, int n_images, float weight_x0,
                  float weight_img, void* scratch, hipStream_t st) {
  const std::string name("srgd_guidance_step");
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!img || !x_start || !cond01 || !images || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (!std::isfinite(weight_x0) || !std::isfinite(weight_img)) SRGD_EXT_FAIL(name + ": weight_x0 and weight_img must be finite");
  if ((((uintptr_t)img | (uintptr_t)x_start | (uintptr_t)cond01) & 3u) != 0) SRGD_EXT_FAIL(name + ": img, x_start and cond01 must be 4-byte aligned");
  if (((uintptr_t)scratch & 255u) != 0) SRGD_EXT_FAIL(name + ": scratch must be 256-byte aligned");
  long long lo = 0, hi = 0, clo = 0, chi = 0;            // the elements the call covers in img / x_start and in cond01
  unsigned long long scr_bytes = 0;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const srgd_guidance_image& m = images[i];
    const long long h = m.h, w = m.w;
    if (h < 5 || w < 5) SRGD_EXT_FAIL(name + ": bad size (h and w must be >= 5: smaller windows overlap and depend on the size)");
    if (m.Hp < 1 || m.Wp < 1 || 3ll * m.Hp * m.Wp >= (1ll << 31)) SRGD_EXT_FAIL(name + ": bad canvas (3*Hp*Wp must be in 1 .. 2^31 - 1)");
    if (m.top < 0 || m.left < 0 || m.top + 4 * h > m.Hp || m.left + 4 * w > m.Wp) SRGD_EXT_FAIL(name + ": the crop box leaves its canvas");
    if (m.canvas_off < 0 || m.canvas_off >= (1ll << 40) || m.cond_off < 0 || m.cond_off >= (1ll << 40))
      SRGD_EXT_FAIL(name + ": offset outside [0, 2^40)");
    const long long canvas = 3ll * m.Hp * m.Wp, planes = 48 * h * w;
    lo = i == 0 ? m.canvas_off : std::min<long long>(lo, m.canvas_off);
    hi = i == 0 ? m.canvas_off + canvas : std::max<long long>(hi, m.canvas_off + canvas);
    clo = i == 0 ? m.cond_off : std::min<long long>(clo, m.cond_off);
    chi = i == 0 ? m.cond_off + planes : std::max<long long>(chi, m.cond_off + planes);
    scr_bytes += gd_scratch(h, w);
  }
  for (int i = 0; i < n_images; ++i)
    for (int j = i + 1; j < n_images; ++j) {
      const Range a{images[i].canvas_off, images[i].canvas_off + 3ll * images[i].Hp * images[i].Wp};
      const Range b{images[j].canvas_off, images[j].canvas_off + 3ll * images[j].Hp * images[j].Wp};
      if (a.meets(b)) SRGD_EXT_FAIL(name + ": overlapping canvases");
    }
  const Range r_img{(long long)(intptr_t)img + 4 * lo, (long long)(intptr_t)img + 4 * hi};
  const Range r_xs{(long long)(intptr_t)x_start + 4 * lo, (long long)(intptr_t)x_start + 4 * hi};
  const Range r_cond{(long long)(intptr_t)cond01 + 4 * clo, (long long)(intptr_t)cond01 + 4 * chi};
  const Range r_scr{(long long)(intptr_t)scratch, (long long)(intptr_t)scratch + (long long)scr_bytes};
  if (r_img.meets(r_xs) || r_img.meets(r_cond) || r_img.meets(r_scr) || r_xs.meets(r_cond) || r_xs.meets(r_scr) || r_cond.meets(r_scr))
    SRGD_EXT_FAIL(name + ": overlapping buffers (img, x_start, cond01 and scratch are disjoint)");
  static const GdDown down = framed_down_vectors();
  static const GdUp up = framed_up_vectors();
  unsigned long long scr = 0;                            // the images' D, packed in image order (floats)
  for (int first = 0; first < n_images; first += GD_MAX_IMAGES) {     // one launch sequence per GD_MAX_IMAGES images
    const int cnt = std::min(GD_MAX_IMAGES, n_images - first);
    GdTable tab;
    unsigned max_tiles = 0;
    for (int k = 0; k < GD_MAX_IMAGES; ++k) tab.im[k] = GdImage{0ll, 0ll, 0ull, 0, 0, 0, 0};
    for (int k = 0; k < cnt; ++k) {
      const srgd_guidance_image& m = images[first + k];
      tab.im[k] = GdImage{m.canvas_off + (long long)m.top * m.Wp + m.left, m.cond_off, scr, m.Hp * m.Wp, m.Wp, m.h, m.w};
      scr += gd_scratch(m.h, m.w) / 4;
      max_tiles = std::max(max_tiles, gd_tiles_x(m.w) * gd_tiles_y(m.h));
    }
    const dim3 tiles(max_tiles, (unsigned)cnt, 3u);
    hipLaunchKernelGGL(guidance_reduce_kernel, tiles, dim3(GD_THREADS), 0, st, tab, down, (const float*)x_start, (float*)scratch);
    hipLaunchKernelGGL(guidance_update_kernel, tiles, dim3(GD_THREADS), 0, st, tab, up, img, x_start, cond01, (const float*)scratch,
                       weight_x0, weight_img);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_guidance_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_guidance_coeffs(float down[5][16], float up[16][4]) {
  if (!down || !up) SRGD_EXT_FAIL("srgd_guidance_coeffs: null argument");
  const GdDown d = framed_down_vectors();
  const GdUp u = framed_up_vectors();
  for (int v = 0; v < 5; ++v)
    for (int t = 0; t < GD_RTAPS; ++t) down[v][t] = d.k[v][t];
  for (int v = 0; v < 16; ++v)
    for (int t = 0; t < GD_UTAPS; ++t) up[v][t] = u.k[v][t];
  return 0;
}

SRGD_EXT_EXPORT int srgd_guidance_step(float* img, float* x_start, const float* cond01, const srgd_guidance_image* images_host, int n_images,
                                       float weight_x0, float weight_img, void* scratch, void* stream) {
  return guidance_step(img, x_start, cond01, images_host, n_images, weight_x0, weight_img, scratch, (hipStream_t)stream);
}

}  // extern "C"
