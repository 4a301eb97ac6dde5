// Image front/back end of the sampling path on the GPU (reference inference.py:66-73, :93):
//   * x4 (any integer or fractional factor) bicubic upsample of an 8-bit RGB image, bit-exact with Pillow's
//     Image.resize(BICUBIC) - which is what torchvision's T.Resize does for a PIL input - followed by ToTensor (/255);
//   * ToPILImage of the sampler's output: mul(255) and truncation to uint8.
// Pillow's algorithm (src/libImaging/Resample.c, pinned version 12.2.0 in this image; restated from its published
// source): per output coordinate a window [xmin, xmin+n) of the input (support 2.0 for bicubic, a = -0.5, clipped to
// the image) with double-precision weights renormalised to sum 1, converted to 22-bit fixed point (round half away from
// zero); horizontal pass, rounded and clipped to 8 bits, then vertical pass; accumulators start at 1 << 21 and the
// result is clip8(acc >> 22).  The tables are built on the host exactly as Pillow builds them; the passes are integer
// kernels (HBM-bound byte work, one thread per output sample; no MFMA shape to be had here).
//   * colour correction of the sampler's [0,1] output against its [0,1] bicubic condition (engine extension, absent upstream;
//     arithmetic of StableSR's wavelet_reconstruction / adaptive_instance_normalization, restated from their published source):
//     see "colour fix" below.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/srgd_hip.h"
#include "kernels.hpp"
#include "pillow_coeffs.hpp"

namespace srgd {
namespace {

constexpr int PREC_BITS = PILLOW_PREC_BITS;
constexpr int KSIZE_MAX = 64;
static_assert(KSIZE_MAX <= pillow::MAX_TAPS, "the widest table of pillow_coeffs.hpp");

// Pillow's bicubic table of an axis (pillow_coeffs.hpp).  bounds: [out][2] = (first input index, count); kk: [out][ksize] fixed-point weights
int build_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk, int* ksize_out) {
  const int ksize = pillow::ksize(in_size, out_size, pillow::BICUBIC);
  if (ksize > KSIZE_MAX) SRGD_FAIL("image resize: reduction factor too large for this build");
  bounds.assign((size_t)out_size * 2, 0);
  kk.assign((size_t)out_size * ksize, 0);
  pillow::axis_table(in_size, out_size, pillow::BICUBIC, bounds.data(), kk.data());
  *ksize_out = ksize;
  return 0;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> PREC_BITS;               // arithmetic shift, as Pillow's clip8 lookup index
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// src [h][w][3] u8 -> tmp [h][out_w][3] u8
__global__ void resample_h_kernel(const unsigned char* __restrict__ src, int h, int w, int out_w,
                                  const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                  unsigned char* __restrict__ tmp) {
  const long n = (long)h * out_w * 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long t = i / 3;
    const int xx = (int)(t % out_w), y = (int)(t / out_w);
    const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
    int acc = 1 << (PREC_BITS - 1);
    for (int x = 0; x < cnt; ++x) acc += (int)src[((long)y * w + xmin + x) * 3 + c] * kk[xx * ksize + x];
    tmp[i] = (unsigned char)clip8(acc);
  }
}

// tmp [h][out_w][3] u8 -> dst [3][out_h][out_w] fp32 = u8 / 255 (ToTensor)
__global__ void resample_v_unit_kernel(const unsigned char* __restrict__ tmp, int h, int out_h, int out_w,
                                       const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                       float* __restrict__ dst) {
  const long plane = (long)out_h * out_w;
  const long n = plane * 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = (int)(i / plane);
    const long r = i - (long)c * plane;
    const int yy = (int)(r / out_w), x = (int)(r - (long)yy * out_w);
    const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
    int acc = 1 << (PREC_BITS - 1);
    for (int y = 0; y < cnt; ++y) acc += (int)tmp[((long)(ymin + y) * out_w + x) * 3 + c] * kk[yy * ksize + y];
    dst[i] = __fdiv_rn((float)clip8(acc), 255.0f);
  }
}

// img [3][h][w] fp32 in [0,1] -> dst [h][w][3] u8 : mul(255).byte()
__global__ void unit_to_u8_kernel(const float* __restrict__ img, int h, int w, unsigned char* __restrict__ dst) {
  const long plane = (long)h * w;
  const long n = plane * 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long px = i / 3;
    const float v = __fmul_rn(img[(long)c * plane + px], 255.0f);
    dst[i] = (unsigned char)(int)v;              // truncation toward zero, as Tensor.byte()
  }
}

// ---- colour fix ------------------------------------------------------------------------------------------------------------
// c = sampler output, s = condition, both planar [3][h][w] fp32 in [0,1].
//   wavelet: result = high5(c) + low5(s), five a-trous levels r = 1, 2, 4, 8, 16 of the kernel [1,2,1]^T [1,2,1] / 16 with
//     replicate padding.  A blur with clamped indices is linear, so high5(c) + low5(s) = c + B16(B8(B4(B2(B1(s - c))))): ONE chain on
//     the difference, each B_r separable (0.25 x[clamp(i-r)] + 0.5 x[i] + 0.25 x[clamp(i+r)] along x, then along y) - ten passes.  The
//     levels clamp one by one: clamp(clamp(i + 2k) + j) != clamp(i + 2k + j) next to the border, so they do not fold into one kernel.
//   adain: per channel result = (c - mean_c) / std_c * std_s + mean_s, std = sqrt(unbiased variance + 1e-5); sums and sums of
//     squares in float64 over fixed chunks of CF_CHUNK pixels of a channel plane (a partition of the image's own h * w, whatever the
//     launch), the chunks of a channel summed in a fixed order by one workgroup: no atomics.
// Every value of an image is computed from that image's pixels by an expression that does not depend on the launch shape
// (fp contraction off), so an image comes out bit-identical alone and inside a group.  A NaN passes through every stage, and the
// final clamp keeps it.
// Work split: blockIdx.y = image (its record is uniform per workgroup), x workgroups stride over the image's elements in quads of four
// that are 16-byte aligned in memory where the buffers are (`vec`): the centre tap and the result move as one 16-byte access, the quads
// cut by the ends of the image and the +-r taps as guarded scalars.
struct CfImage {
  long long off;       // first element of the image's planes in every buffer
  long long aux;       // adain: first double of the image's statistics block in the scratch
  int h, w;
};
constexpr int CF_MAX_IMAGES = 128;     // records travel as a kernel argument (3 KiB): no table to upload, nothing to free
struct CfTable { CfImage im[CF_MAX_IMAGES]; };
constexpr unsigned CF_CHUNK = 4096;    // adain: pixels of one partial sum

// One separable pass of one level.  AXIS 0: along x, 1: along y.  FIRST: the input is s - c, formed on the fly; LAST: the result is
// clamp(c + blur) written to dst01 (which may be out01: only the thread's own pixel of c is read here).
template <int AXIS, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void wavelet_pass_kernel(CfTable tab, const float* out01,
                                                           const float* __restrict__ cond01, const float* src, float* dst, int r,
                                                           int vec) {
#pragma clang fp contract(off)
  const CfImage im = tab.im[blockIdx.y];
  const unsigned w = (unsigned)im.w, h = (unsigned)im.h, n = 3u * h * w, ur = (unsigned)r;
  const float* c = out01 + im.off;
  const float* s = cond01 + im.off;
  const float* a = FIRST ? nullptr : src + im.off;
  float* d = dst + im.off;
  const unsigned mis = vec ? (unsigned)(im.off & 3) : 0u;          // elements of the first quad that lie before the image
  const unsigned nquads = (n + mis + 3u) / 4u;
  auto tap = [&](unsigned j) { return FIRST ? s[j] - c[j] : a[j]; };
  for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < nquads; q += gridDim.x * 256u) {
    const unsigned lo = q == 0 ? 0u : 4u * q - mis, hi = std::min(4u * q - mis + 4u, n);     // elements [lo, hi) of this quad
    const bool full = vec && hi - lo == 4u;
    f32x4 ctr = {0.f, 0.f, 0.f, 0.f}, base = {0.f, 0.f, 0.f, 0.f}, res;
    if (full) {
      if (FIRST) ctr = *reinterpret_cast<const f32x4*>(s + lo) - *reinterpret_cast<const f32x4*>(c + lo);
      else ctr = *reinterpret_cast<const f32x4*>(a + lo);
      if (LAST) base = *reinterpret_cast<const f32x4*>(c + lo);
    }
    unsigned row = lo / w, x = lo - row * w, y = AXIS == 1 ? row % h : 0u;   // row counts the 3 h rows of the three planes
#pragma unroll
    for (unsigned k = 0; k < 4u; ++k) {
      const unsigned e = lo + k;
      if (e < hi) {
        const unsigned below = AXIS == 0 ? std::min(ur, x) : std::min(ur, y) * w;
        const unsigned above = AXIS == 0 ? std::min(ur, w - 1u - x) : std::min(ur, h - 1u - y) * w;
        const float m = full ? ctr[k] : tap(e);
        float v = 0.25f * tap(e - below) + 0.5f * m;
        v = v + 0.25f * tap(e + above);
        if (LAST) v = clamp_keep_nan((full ? base[k] : c[e]) + v, 0.0f, 1.0f);
        res[k] = v;
        if (!full) d[e] = v;
        if (++x == w) {
          x = 0;
          if (AXIS == 1 && ++y == h) y = 0;
        }
      }
    }
    if (full) *reinterpret_cast<f32x4*>(d + lo) = res;
  }
}

// adain stage 1: partial (sum c, sum c^2, sum s, sum s^2) in float64 of chunk `idx % nchunks` of channel `idx / nchunks`, stored by
// idx: the partition and the order inside a chunk depend on h * w alone.
__global__ __launch_bounds__(256) void adain_partial_kernel(CfTable tab, const float* __restrict__ out01,
                                                            const float* __restrict__ cond01, double* __restrict__ aux) {
#pragma clang fp contract(off)
  const CfImage im = tab.im[blockIdx.y];
  const unsigned plane = (unsigned)im.h * (unsigned)im.w;
  const unsigned nchunks = (plane + CF_CHUNK - 1u) / CF_CHUNK;
  const float* c = out01 + im.off;
  const float* s = cond01 + im.off;
  double* part = aux + im.aux + 12;                                   // [3][nchunks][4] after the [3][4] statistics
  __shared__ double red[4][4];
  for (unsigned idx = blockIdx.x; idx < 3u * nchunks; idx += gridDim.x) {
    const unsigned ch = idx / nchunks, first = (idx - ch * nchunks) * CF_CHUNK;
    const unsigned last = std::min(first + CF_CHUNK, plane);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (unsigned p = first + threadIdx.x; p < last; p += 256u) {
      const double vc = (double)c[ch * plane + p], vs = (double)s[ch * plane + p];
      acc[0] += vc;
      acc[1] += vc * vc;
      acc[2] += vs;
      acc[3] += vs * vs;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
    }
    __syncthreads();                                                  // the previous chunk's readers are done with red
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < 4u) part[(size_t)idx * 4 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// adain stage 2: one workgroup per (channel, image) sums the channel's partials in a fixed order and leaves
// (mean_c, std_c, mean_s, std_s) as doubles at the head of the image's block.
__global__ __launch_bounds__(256) void adain_stats_kernel(CfTable tab, double* __restrict__ aux) {
#pragma clang fp contract(off)
  const CfImage im = tab.im[blockIdx.y];
  const unsigned plane = (unsigned)im.h * (unsigned)im.w;
  const unsigned nchunks = (plane + CF_CHUNK - 1u) / CF_CHUNK;
  const unsigned ch = blockIdx.x;
  const double* part = aux + im.aux + 12 + (size_t)ch * nchunks * 4;
  __shared__ double red[4][4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (unsigned k = threadIdx.x; k < nchunks; k += 256u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += part[(size_t)k * 4 + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) red[threadIdx.x >> 6][j] = acc[j];
  }
  __syncthreads();
  if (threadIdx.x < 2u) {                                             // thread 0: c, thread 1: s
    const int j = 2 * (int)threadIdx.x;
    const double sum = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    const double sq = (red[0][j + 1] + red[1][j + 1]) + (red[2][j + 1] + red[3][j + 1]);
    const double cnt = (double)plane;
    const double mean = sum / cnt;
    const double var = (sq - sum * mean) / (cnt - 1.0);               // unbiased; one pixel: 0 / 0 = NaN, as torch.var
    aux[im.aux + ch * 4 + j] = mean;
    aux[im.aux + ch * 4 + j + 1] = sqrt(var + 1e-5);
  }
}

// adain stage 3: dst = clamp((c - mean_c) / std_c * std_s + mean_s), fp32 with the statistics rounded to fp32.
__global__ __launch_bounds__(256) void adain_apply_kernel(CfTable tab, const float* out01, const double* __restrict__ aux,
                                                          float* dst, int vec) {
#pragma clang fp contract(off)
  const CfImage im = tab.im[blockIdx.y];
  const unsigned plane = (unsigned)im.h * (unsigned)im.w, n = 3u * plane;
  const float* c = out01 + im.off;
  float* d = dst + im.off;
  const double* st = aux + im.aux;
  const unsigned mis = vec ? (unsigned)(im.off & 3) : 0u;
  const unsigned nquads = (n + mis + 3u) / 4u;
  for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < nquads; q += gridDim.x * 256u) {
    const unsigned lo = q == 0 ? 0u : 4u * q - mis, hi = std::min(4u * q - mis + 4u, n);
    const bool full = vec && hi - lo == 4u;
    f32x4 in = {0.f, 0.f, 0.f, 0.f}, res;
    if (full) in = *reinterpret_cast<const f32x4*>(c + lo);
    unsigned ch = lo / plane, left = (ch + 1u) * plane - lo;          // elements of channel ch from lo on
    float mc = (float)st[ch * 4], sc = (float)st[ch * 4 + 1], ms = (float)st[ch * 4 + 2], ss = (float)st[ch * 4 + 3];
#pragma unroll
    for (unsigned k = 0; k < 4u; ++k) {
      const unsigned e = lo + k;
      if (e < hi) {
        float v = __fdiv_rn((full ? in[k] : c[e]) - mc, sc) * ss;
        v = clamp_keep_nan(v + ms, 0.0f, 1.0f);
        res[k] = v;
        if (!full) d[e] = v;
        if (--left == 0u && e + 1u < n) {                             // the quad runs on into the next channel
          ++ch;
          left = plane;
          mc = (float)st[ch * 4], sc = (float)st[ch * 4 + 1], ms = (float)st[ch * 4 + 2], ss = (float)st[ch * 4 + 3];
        }
      }
    }
    if (full) *reinterpret_cast<f32x4*>(d + lo) = res;
  }
}

int cf_grid(unsigned long long work_items) { return (int)std::min<unsigned long long>((work_items + 255) / 256, 256ull * 32); }

template <int AXIS, bool FIRST, bool LAST>
void launch_wavelet_pass(dim3 grid, hipStream_t st, const CfTable& tab, const float* out01, const float* cond01, const float* src,
                         float* dst, int r, int vec) {
  hipLaunchKernelGGL((wavelet_pass_kernel<AXIS, FIRST, LAST>), grid, dim3(256), 0, st, tab, out01, cond01, src, dst, r, vec);
}

int color_fix_images(const char* who, const float* out01, const float* cond01, const int64_t* offsets, const int32_t* hw, int n_images,
                     int mode, float* dst01, float* scratch, hipStream_t st) {
  const std::string name(who);
  if (!out01 || !cond01 || !offsets || !hw || !dst01 || !scratch) SRGD_FAIL(name + ": null argument");
  if (n_images < 1) SRGD_FAIL(name + ": n_images must be >= 1");
  if (mode != 1 && mode != 2) SRGD_FAIL(name + ": unknown mode (1 = wavelet, 2 = adain)");
  if (dst01 == cond01) SRGD_FAIL(name + ": dst01 may alias out01, not cond01");
  long long extent = 0;
  for (int i = 0; i < n_images; ++i) {
    const long long h = hw[2 * i], w = hw[2 * i + 1];
    if (h < 1 || w < 1) SRGD_FAIL(name + ": bad size");
    if (offsets[i] < 0) SRGD_FAIL(name + ": negative offset");
    if (3 * h * w > 0x7fffff00ll) SRGD_FAIL(name + ": image of more than 2^31 elements");
    extent = std::max(extent, (long long)offsets[i] + 3 * h * w);
  }
  extent = (extent + 3) & ~3ll;
  auto aligned16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  const int vec = aligned16(out01) && aligned16(cond01) && aligned16(dst01) && aligned16(scratch) ? 1 : 0;
  if (mode == 2 && ((uintptr_t)scratch & 7u) != 0) SRGD_FAIL(name + ": adain needs an 8-byte aligned scratch");
  long long aux = 0;                                     // adain statistics blocks, packed in image order
  for (int first = 0; first < n_images; first += CF_MAX_IMAGES) {       // one launch sequence per CF_MAX_IMAGES images
    const int cnt = std::min(CF_MAX_IMAGES, n_images - first);
    CfTable tab;
    unsigned long long max_n = 0, max_chunks = 0;
    for (int k = 0; k < cnt; ++k) {
      const int i = first + k;
      const unsigned long long plane = (unsigned long long)hw[2 * i] * (unsigned long long)hw[2 * i + 1];
      const unsigned long long chunks = (plane + CF_CHUNK - 1) / CF_CHUNK;
      tab.im[k] = CfImage{(long long)offsets[i], aux, hw[2 * i], hw[2 * i + 1]};
      aux += 12 * (1 + (long long)chunks);
      max_n = std::max(max_n, 3 * plane);
      max_chunks = std::max(max_chunks, chunks);
    }
    for (int k = cnt; k < CF_MAX_IMAGES; ++k) tab.im[k] = CfImage{0, 0, 0, 0};
    const dim3 grid((unsigned)cf_grid(max_n / 4 + 2), (unsigned)cnt);
    if (mode == 1) {
      float* a = scratch;
      float* b = scratch + extent;
      launch_wavelet_pass<0, true, false>(grid, st, tab, out01, cond01, nullptr, a, 1, vec);
      launch_wavelet_pass<1, false, false>(grid, st, tab, out01, cond01, a, b, 1, vec);
      for (int r = 2; r <= 16; r *= 2) {
        launch_wavelet_pass<0, false, false>(grid, st, tab, out01, cond01, b, a, r, vec);
        if (r < 16) launch_wavelet_pass<1, false, false>(grid, st, tab, out01, cond01, a, b, r, vec);
      }
      launch_wavelet_pass<1, false, true>(grid, st, tab, out01, cond01, a, dst01, 16, vec);
    } else {
      double* stats = reinterpret_cast<double*>(scratch);
      const dim3 pgrid((unsigned)std::min<unsigned long long>(3 * max_chunks, 256ull * 32), (unsigned)cnt);
      hipLaunchKernelGGL(adain_partial_kernel, pgrid, dim3(256), 0, st, tab, out01, cond01, stats);
      hipLaunchKernelGGL(adain_stats_kernel, dim3(3, (unsigned)cnt), dim3(256), 0, st, tab, stats);
      hipLaunchKernelGGL(adain_apply_kernel, grid, dim3(256), 0, st, tab, out01, stats, dst01, vec);
    }
    SRGD_HIP(hipGetLastError());
  }
  return 0;
}

int grid1d(long n) { return (int)std::min<long>((n + 255) / 256, 256L * 32); }

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

int srgd_image_resize_bicubic_u8(const uint8_t* src_hwc, int h, int w, int out_h, int out_w, float* dst01_chw,
                                 void* stream) {
  if (!src_hwc || !dst01_chw) SRGD_FAIL("srgd_image_resize_bicubic_u8: null argument");
  if (h < 1 || w < 1 || out_h < 1 || out_w < 1) SRGD_FAIL("srgd_image_resize_bicubic_u8: bad size");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int> bw, kw, bh, kh;
  int ksw = 0, ksh = 0;
  SRGD_TRY(build_coeffs(w, out_w, bw, kw, &ksw));
  SRGD_TRY(build_coeffs(h, out_h, bh, kh, &ksh));
  // one scratch allocation: [tmp u8 | tables]; released after the stream has drained (once per image, off the hot loop)
  const size_t tmp_bytes = ((size_t)h * out_w * 3 + 255) & ~(size_t)255;
  const size_t tab_ints = bw.size() + kw.size() + bh.size() + kh.size();
  char* scratch = nullptr;
  SRGD_HIP(hipMalloc((void**)&scratch, tmp_bytes + tab_ints * 4));
  int* d_bw = reinterpret_cast<int*>(scratch + tmp_bytes);
  int* d_kw = d_bw + bw.size();
  int* d_bh = d_kw + kw.size();
  int* d_kh = d_bh + bh.size();
  hipError_t err = hipSuccess;
  auto up = [&](int* d, const std::vector<int>& v) {
    if (err == hipSuccess) err = hipMemcpyAsync(d, v.data(), v.size() * 4, hipMemcpyHostToDevice, st);
  };
  up(d_bw, bw); up(d_kw, kw); up(d_bh, bh); up(d_kh, kh);
  if (err == hipSuccess) {
    unsigned char* tmp = reinterpret_cast<unsigned char*>(scratch);
    hipLaunchKernelGGL(resample_h_kernel, dim3(grid1d((long)h * out_w * 3)), dim3(256), 0, st, src_hwc, h, w, out_w, d_bw,
                       d_kw, ksw, tmp);
    hipLaunchKernelGGL(resample_v_unit_kernel, dim3(grid1d((long)out_h * out_w * 3)), dim3(256), 0, st, tmp, h, out_h,
                       out_w, d_bh, d_kh, ksh, dst01_chw);
    err = hipGetLastError();
  }
  const hipError_t serr = hipStreamSynchronize(st);      // host tables and the scratch must outlive the copies / kernels
  (void)hipFree(scratch);
  if (err != hipSuccess) SRGD_FAIL(std::string("srgd_image_resize_bicubic_u8: ") + hipGetErrorString(err));
  if (serr != hipSuccess) SRGD_FAIL(std::string("srgd_image_resize_bicubic_u8: ") + hipGetErrorString(serr));
  return 0;
}

int srgd_image_unit_to_u8(const float* img01_chw, int h, int w, uint8_t* dst_hwc, void* stream) {
  if (!img01_chw || !dst_hwc) SRGD_FAIL("srgd_image_unit_to_u8: null argument");
  if (h < 1 || w < 1) SRGD_FAIL("srgd_image_unit_to_u8: bad size");
  hipLaunchKernelGGL(unit_to_u8_kernel, dim3(grid1d((long)h * w * 3)), dim3(256), 0, (hipStream_t)stream, img01_chw, h, w,
                     dst_hwc);
  SRGD_HIP(hipGetLastError());
  return 0;
}

int srgd_image_color_fix(const float* out01, const float* cond01, int h, int w, int mode, float* dst01, float* scratch,
                         void* stream) {
  const int64_t off = 0;
  const int32_t hw[2] = {h, w};
  return color_fix_images("srgd_image_color_fix", out01, cond01, &off, hw, 1, mode, dst01, scratch, (hipStream_t)stream);
}

int srgd_image_color_fix_images(const float* out01, const float* cond01, const int64_t* offsets_host, const int32_t* hw_host,
                                int n_images, int mode, float* dst01, float* scratch, void* stream) {
  return color_fix_images("srgd_image_color_fix_images", out01, cond01, offsets_host, hw_host, n_images, mode, dst01, scratch,
                          (hipStream_t)stream);
}

}  // extern "C"
