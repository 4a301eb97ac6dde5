// Quality numbers of a sampler output against its ground truth on the GPU (engine extension, absent upstream): Y-channel PSNR, RGB
// PSNR and Y-channel SSIM with a border crop - the protocol of the x4 super-resolution literature (BasicSR's calculate_psnr /
// calculate_ssim with test_y_channel, MATLAB's rgb2ycbcr and ssim), restated from their published definitions.
//
// Definition, per image.  out01: fp32 planar [3][h][w], the engine's [0,1] output (after the colour fix where one ran); ref_u8: uint8
// [h][w][3], the ground-truth image as decoded; crop >= 0: both lose `crop` pixels on every side before anything is computed
// (ch = h - 2 crop, cw = w - 2 crop).
//   quantisation: q = (int)(out01 * 255.0f), unit_to_u8_kernel's fp32 product and truncation (imageio.hip), so the numbers describe the
//     PNG on disk.  Everything after it is float64 with contraction off.
//   luma: Y = 65.481 (R/255) + 128.553 (G/255) + 24.966 (B/255) + 16 (BT.601, MATLAB rgb2ycbcr / BasicSR), not rounded.
//   psnr_y = 10 log10(255^2 / mean((Yo - Yr)^2)) over the ch x cw pixels; psnr_rgb the same over the 3 ch cw quantised channel values;
//     a mean of exactly 0 gives +inf.
//   ssim_y: 11x11 Gaussian window, sigma 1.5: weights exp(-(i-5)^2 / 4.5), i = 0..10, normalised to sum 1 in float64, applied
//     separably (along x, then along y), over the valid region only: vh x vw = (ch - 10) x (cw - 10) positions.  C1 = (0.01*255)^2,
//     C2 = (0.03*255)^2.  Per position ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)) with mx, my the filtered
//     lumas and sxx = filtered x^2 - mx^2, syy, sxy likewise; ssim_y is the mean of the map.
//   non-finite values: an out01 value inside the cropped region that is NaN or +-Inf makes all three numbers of THAT image NaN (the
//     test runs before the integer conversion, which is undefined for it); the fourth result is the count of such values.  One in the
//     cropped-off border is never read.
//   ch < 11 or cw < 11: no SSIM position - an error, nothing is launched.
//
// Work split.  The SSIM positions of an image are cut into fixed tiles of MX_TW x MX_TH (32 x 8, one position per thread of a
// 256-thread workgroup): tile (tx, ty) of ceil(vw / 32) x ceil(vh / 8).  blockIdx.y is the image (its record travels in the kernel
// argument, as CfTable does: no table upload), blockIdx.x strides over the image's tiles.  A tile stages the two luma patches, tile +
// 10-pixel halo (18 x 42), as float64 in LDS, runs the 11-tap pass along x over (x, y, x^2, y^2, xy) into LDS (18 x 32 x 5), then the
// pass along y, one SSIM value per thread.  Every cropped pixel is owned by exactly one tile - the tile whose 32 x 8 box holds it, the
// last tile column and row also taking the 10 pixels beyond their box, which their halo covers - and the owner adds its squared errors
// (Y and RGB) and its non-finite count while staging.  The four sums of a tile are reduced in a fixed order (the thread's own pixels in
// patch order, xor-shuffles over the wave, the four waves as (0+1)+(2+3)) into one record of four doubles, stored plainly: no
// atomics.  A second kernel, one workgroup per image, adds the image's records - thread t the records t, t+256, ... in index order,
// then the same tree - and writes psnr_y, psnr_rgb, ssim_y, n_nonfinite.  Tiles, ownership and both orders depend on (h, w, crop)
// alone: not on the grid, not on the image's offsets, not on its neighbours in the group - an image's four doubles are bit-identical
// alone and in any group.
// LDS: a 32-lane group of a float64 access (ds_read_b64: banks (a/4) mod 64, two groups of 32 lanes) is one tile row, 32 consecutive
// doubles = 64 consecutive banks, conflict-free at any row stride, in both passes; that is why the tile is 32 wide and not 16 x 16,
// whose two rows per group would need a row stride of 16 mod 32 doubles.  12,096 B (patches) + 23,040 B (x pass) + 128 B = 35,264 B per
// workgroup: four workgroups per CU.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_metrics.h"
#include "ext_common.hpp"

// This file is a library of its own (libsrgd_metrics.so, include/srgd_metrics.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing (pillow_resample.hpp and pillow_x4.hpp, the code some of them have in
// common, are headers too: no symbol is shared).
namespace srgd {
namespace {

constexpr int MX_TW = 32, MX_TH = 8;                 // SSIM positions of a tile: one per thread
constexpr int MX_TAPS = 11, MX_HALO = MX_TAPS - 1;
constexpr int MX_PW = MX_TW + MX_HALO, MX_PH = MX_TH + MX_HALO;
constexpr int MX_MAX_IMAGES = 128;                   // records travel as a kernel argument (3.5 KiB)
constexpr unsigned MX_MAX_GRID_X = 8192;

struct MxTable {
  long long out_off[MX_MAX_IMAGES];                  // first element of the image's planes in out01
  long long ref_off[MX_MAX_IMAGES];                  // first byte of the image in ref_u8
  int h[MX_MAX_IMAGES], w[MX_MAX_IMAGES];
  unsigned part[MX_MAX_IMAGES];                      // first record (four doubles each) of the image in the scratch
};
struct MxWindow { double g[MX_TAPS]; };

// Sum over the workgroup of v[0..3] in a fixed order: xor-shuffles over each wave into red[wave], a barrier, then mx_total(red, j) in
// whichever thread wants sum j.  The caller keeps red untouched until its readers have passed another barrier.
__device__ __forceinline__ void mx_block_reduce(double (&v)[4], double (*red)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) red[threadIdx.x >> 6][j] = v[j];
  }
  __syncthreads();
}
__device__ __forceinline__ double mx_total(const double (*red)[4], unsigned j) { return (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]); }

__global__ __launch_bounds__(256) void metrics_tile_kernel(MxTable tab, MxWindow win, const float* __restrict__ out01,
                                                           const unsigned char* __restrict__ ref_u8, int crop,
                                                           double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double pa[MX_PH][MX_PW], pb[MX_PH][MX_PW];          // luma of the output / of the reference
  __shared__ double hb[5][MX_PH][MX_TW];                         // the pass along x of x, y, x^2, y^2, xy
  __shared__ double red[4][4];
  const unsigned im = blockIdx.y;
  const int h = tab.h[im], w = tab.w[im];
  const int ch = h - 2 * crop, cw = w - 2 * crop, vh = ch - MX_HALO, vw = cw - MX_HALO;
  const unsigned ntx = (unsigned)(vw + MX_TW - 1) / MX_TW, nty = (unsigned)(vh + MX_TH - 1) / MX_TH, ntiles = ntx * nty;
  const long long plane = (long long)h * w;
  const float* o = out01 + tab.out_off[im];
  const unsigned char* r = ref_u8 + tab.ref_off[im];
  double* part = partials + 4ull * tab.part[im];
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const unsigned ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = (int)ty * MX_TH, x0 = (int)tx * MX_TW;       // cropped coordinates of the tile's first position and pixel
    const int own_h = ty == nty - 1 ? ch - y0 : MX_TH, own_w = tx == ntx - 1 ? cw - x0 : MX_TW;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                       // ssim, squared error Y, squared error RGB, non-finite values
    for (int idx = (int)threadIdx.x; idx < MX_PH * MX_PW; idx += 256) {
      const int py = idx / MX_PW, px = idx - py * MX_PW;
      const int cy = y0 + py, cx = x0 + px;
      double yo = 0.0, yr = 0.0;
      if (cy < ch && cx < cw) {                                 // inside the cropped image: rows crop .. h-crop-1 of the buffers
        const long long pix = (long long)(cy + crop) * w + (cx + crop);
        int q[3], g[3], bad = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = o[c * plane + pix];
          const bool fin = __builtin_isfinite(v);
          bad += fin ? 0 : 1;
          q[c] = fin ? (int)__fmul_rn(v, 255.0f) : 0;
          g[c] = (int)r[pix * 3 + c];
        }
        yo = 65.481 * ((double)q[0] / 255.0) + 128.553 * ((double)q[1] / 255.0) + 24.966 * ((double)q[2] / 255.0) + 16.0;
        yr = 65.481 * ((double)g[0] / 255.0) + 128.553 * ((double)g[1] / 255.0) + 24.966 * ((double)g[2] / 255.0) + 16.0;
        if (py < own_h && px < own_w) {
          const double d = yo - yr;
          acc[1] += d * d;
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[2] += (double)((q[c] - g[c]) * (q[c] - g[c]));
          acc[3] += (double)bad;
        }
      }
      pa[py][px] = yo;
      pb[py][px] = yr;
    }
    __syncthreads();
    for (int idx = (int)threadIdx.x; idx < MX_PH * MX_TW; idx += 256) {
      const int py = idx / MX_TW, x = idx - py * MX_TW;
      double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < MX_TAPS; ++k) {
        const double a = pa[py][x + k], b = pb[py][x + k], gk = win.g[k];
        s[0] += gk * a;
        s[1] += gk * b;
        s[2] += gk * (a * a);
        s[3] += gk * (b * b);
        s[4] += gk * (a * b);
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) hb[j][py][x] = s[j];
    }
    __syncthreads();
    {
      const int x = (int)(threadIdx.x & (MX_TW - 1)), y = (int)(threadIdx.x / MX_TW);
      double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < MX_TAPS; ++k) {
        const double gk = win.g[k];
#pragma unroll
        for (int j = 0; j < 5; ++j) s[j] += gk * hb[j][y + k][x];
      }
      if (y0 + y < vh && x0 + x < vw) {
        const double mx = s[0], my = s[1];
        const double sxx = s[2] - mx * mx, syy = s[3] - my * my, sxy = s[4] - mx * my;
        acc[0] = ((2.0 * mx * my + C1) * (2.0 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2));
      }
    }
    mx_block_reduce(acc, red);                                  // red is written again two barriers further on
    if (threadIdx.x < 4u) part[(size_t)tile * 4 + threadIdx.x] = mx_total(red, threadIdx.x);
  }
}

// One workgroup per image: the image's records summed in a fixed order, then the three numbers.
__global__ __launch_bounds__(256) void metrics_finish_kernel(MxTable tab, int crop, const double* __restrict__ partials,
                                                             double* __restrict__ results) {
#pragma clang fp contract(off)
  __shared__ double red[4][4];
  const unsigned im = blockIdx.x;
  const int ch = tab.h[im] - 2 * crop, cw = tab.w[im] - 2 * crop, vh = ch - MX_HALO, vw = cw - MX_HALO;
  const unsigned ntiles = ((unsigned)(vw + MX_TW - 1) / MX_TW) * ((unsigned)(vh + MX_TH - 1) / MX_TH);
  const double* part = partials + 4ull * tab.part[im];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (unsigned k = threadIdx.x; k < ntiles; k += 256u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += part[(size_t)k * 4 + j];
  }
  mx_block_reduce(acc, red);
  if (threadIdx.x == 0u) {
    const double ssim_sum = mx_total(red, 0), se_y = mx_total(red, 1), se_rgb = mx_total(red, 2), bad = mx_total(red, 3);
    const double npix = (double)ch * (double)cw;
    const double mse_y = se_y / npix, mse_rgb = se_rgb / (3.0 * npix);
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    double psnr_y = mse_y == 0.0 ? inf : 10.0 * log10(255.0 * 255.0 / mse_y);
    double psnr_rgb = mse_rgb == 0.0 ? inf : 10.0 * log10(255.0 * 255.0 / mse_rgb);
    double ssim = ssim_sum / ((double)vh * (double)vw);
    if (bad > 0.0) psnr_y = psnr_rgb = ssim = nan;
    double* res = results + (size_t)im * 4;
    res[0] = psnr_y;
    res[1] = psnr_rgb;
    res[2] = ssim;
    res[3] = bad;
  }
}

int metrics_images(const char* who, const float* out01, const uint8_t* ref_u8, const int64_t* out_offsets, const int64_t* ref_offsets,
                   const int32_t* hw, int n_images, int crop, double* results, double* scratch, hipStream_t st) {
  const std::string name(who);
  if (n_images == 0) return 0;
  if (n_images < 0) SRGD_EXT_FAIL(name + ": n_images must be >= 0");
  if (!out01 || !ref_u8 || !out_offsets || !ref_offsets || !hw || !results || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (crop < 0 || crop > (1 << 20)) SRGD_EXT_FAIL(name + ": bad crop");
  if ((((uintptr_t)results | (uintptr_t)scratch) & 7u) != 0) SRGD_EXT_FAIL(name + ": results and scratch must be 8-byte aligned");
  auto tiles_of = [crop](long long h, long long w) {
    return ((w - 2 * crop - MX_HALO + MX_TW - 1) / MX_TW) * ((h - 2 * crop - MX_HALO + MX_TH - 1) / MX_TH);
  };
  unsigned long long total = 0;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const long long h = hw[2 * i], w = hw[2 * i + 1];
    if (h < 1 || w < 1) SRGD_EXT_FAIL(name + ": bad size");
    if (out_offsets[i] < 0 || ref_offsets[i] < 0) SRGD_EXT_FAIL(name + ": negative offset");
    if (3 * h * w > 0x7fffff00ll) SRGD_EXT_FAIL(name + ": image of more than 2^31 elements");
    if (h - 2 * crop < MX_TAPS || w - 2 * crop < MX_TAPS)
      SRGD_EXT_FAIL(name + ": an image needs at least 11 x 11 pixels inside the crop (no SSIM position otherwise)");
    total += (unsigned long long)tiles_of(h, w);
  }
  if (total > 0xffffffffull) SRGD_EXT_FAIL(name + ": more than 2^32 tiles in one call");
  MxWindow win;
  double sum = 0.0;
  for (int k = 0; k < MX_TAPS; ++k) {
    win.g[k] = std::exp(-(double)((k - 5) * (k - 5)) / 4.5);
    sum += win.g[k];
  }
  for (int k = 0; k < MX_TAPS; ++k) win.g[k] /= sum;
  unsigned part = 0;                                     // records, packed in image order
  for (int first = 0; first < n_images; first += MX_MAX_IMAGES) {     // one launch sequence per MX_MAX_IMAGES images
    const int cnt = std::min(MX_MAX_IMAGES, n_images - first);
    MxTable tab;
    unsigned max_tiles = 0;
    for (int k = 0; k < MX_MAX_IMAGES; ++k) {
      tab.out_off[k] = tab.ref_off[k] = 0;
      tab.h[k] = tab.w[k] = 0;
      tab.part[k] = 0;
    }
    for (int k = 0; k < cnt; ++k) {
      const int i = first + k;
      const unsigned tiles = (unsigned)tiles_of(hw[2 * i], hw[2 * i + 1]);
      tab.out_off[k] = (long long)out_offsets[i];
      tab.ref_off[k] = (long long)ref_offsets[i];
      tab.h[k] = hw[2 * i];
      tab.w[k] = hw[2 * i + 1];
      tab.part[k] = part;
      part += tiles;
      max_tiles = std::max(max_tiles, tiles);
    }
    hipLaunchKernelGGL(metrics_tile_kernel, dim3(std::min(max_tiles, MX_MAX_GRID_X), (unsigned)cnt), dim3(256), 0, st, tab, win, out01,
                       ref_u8, crop, scratch);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)cnt), dim3(256), 0, st, tab, crop, scratch, results + (size_t)first * 4);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_image_metrics_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_image_metrics(const float* out01, const uint8_t* ref_u8, int h, int w, int crop, double* results, double* scratch,
                             void* stream) {
  const int64_t off = 0;
  const int32_t hw[2] = {h, w};
  return metrics_images("srgd_image_metrics", out01, ref_u8, &off, &off, hw, 1, crop, results, scratch, (hipStream_t)stream);
}

SRGD_EXT_EXPORT int srgd_image_metrics_images(const float* out01, const uint8_t* ref_u8, const int64_t* out_offsets_host,
                                    const int64_t* ref_offsets_host, const int32_t* hw_host, int n_images, int crop, double* results,
                                    double* scratch, void* stream) {
  return metrics_images("srgd_image_metrics_images", out01, ref_u8, out_offsets_host, ref_offsets_host, hw_host, n_images, crop,
                        results, scratch, (hipStream_t)stream);
}

}  // extern "C"
