// Mean image and spread map of the K samples of an image on the GPU (engine extension, absent upstream): what K samples of a
// diffusion super-resolver are drawn for.  The inputs are uint8 samples AS SAVED, so every output but one averaged scalar is an exact
// function of integers; the definition is fixed in include/srgd_ensemble.h and restated here in short.
//
// Definition, per element (3 h w of them per image), x_k its K values, 2 <= K <= 256:
//   S = sum x_k, Q = sum x_k^2, D = K Q - S^2 (>= 0, 64-bit);  mean m = (2 S + K) div (2 K);  spread s = twice the population standard
//   deviation sqrt(D) / K rounded to nearest, halves up, by integers: s = 0 if 16 D < K^2, else (2s-1)^2 K^2 <= 16 D < (2s+1)^2 K^2;
//   mean01 = (float)m / 255.0f, planar;  per image mean_std = (sum_e sqrt((double)D_e) / K) / (3 h w), max_std = sqrt((double)max D) / K.
//
// Work split.  An HBM-streaming kernel: (K + 2) bytes of traffic per element (+ 4 with mean01) against a few dozen integer
// instructions.  The 3 h w bytes of an image are cut into vectors of 16 consecutive bytes, one per lane, and chunks of 256 vectors
// (4096 bytes), one per workgroup pass: a wave reads 1 KiB contiguous per sample with one 16-byte load per lane and writes 1 KiB of
// mean and of spread with one 16-byte store each.  The layout contract makes the loads aligned: sample k of an image begins at its
// offset + k * stride, stride = 3 h w rounded up to 16, offsets multiples of 16.  The one partial vector at the end of an image (3 h w
// mod 16 bytes) is read and written byte by byte under a guard: padding is never read or written.  blockIdx.y is the image (its
// record travels in the kernel argument: no table upload), blockIdx.x strides over the image's chunks.
// mean01 transposes HWC to planar: a wave puts its 1 KiB of mean bytes into LDS and then walks the three planes one after the other,
// lane l taking pixel p0 + l, p0 + l + 64, ... of the pixels whose channel-c byte the wave holds - every store instruction of a wave
// writes 64 consecutive floats of one plane.  An element belongs to exactly one wave, so every float is written exactly once.
// Statistics: a lane adds sqrt((double)D) over its 16 elements in element order (elements past the end have D = 0 and add +0.0),
// xor-shuffles add the wave, the four waves are added as (0+1)+(2+3): one record {sum, max D} per chunk, stored plainly.  A second
// kernel, one workgroup per image, adds the records - thread t the records t, t + 256, ... in index order, then the same tree.  No
// atomics; chunks and both orders depend on (h, w) alone - not on the grid, the image's offsets or its neighbours in the group: an
// image's bytes and its two doubles are bit-identical alone and in any group.
// Integer division: 2 S + K < 2^17 and 2 K <= 512, so (2 S + K) div (2 K) = mulhi(2 S + K, floor(2^32 / (2 K)) + 1) exactly (the
// error term (2 S + K) * (M * 2 K - 2^32) <= 2^17 * 2^9 is below 2^32); the host passes M.
#include <algorithm>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_ensemble.h"
#include "ext_common.hpp"

// This file is a library of its own (libsrgd_ensemble.so, include/srgd_ensemble.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing (pillow_resample.hpp and pillow_x4.hpp, the code some of them have in
// common, are headers too: no symbol is shared).
namespace srgd {
namespace {

constexpr int EN_VEC = 16;                           // bytes of a lane per sample: one 16-byte load
constexpr int EN_THREADS = 256;
constexpr unsigned EN_CHUNK = EN_VEC * EN_THREADS;   // elements of a workgroup pass = of one {sum, max} record
constexpr unsigned EN_WAVE = EN_VEC * 64;            // elements of a wave
constexpr int EN_MAX_IMAGES = 128;                   // records travel as a kernel argument (3 KiB)
constexpr unsigned EN_MAX_GRID_X = 8192;

struct EnImage {
  long long m01_off;                                 // first element of the image's planes in mean01
  unsigned in_off16, out_off16;                      // first byte of sample 0 / of the outputs, in units of 16 bytes
  unsigned n;                                        // 3 h w
  unsigned part;                                     // first record (two 8-byte words each) of the image in the scratch
};
struct EnTable { EnImage im[EN_MAX_IMAGES]; };

__device__ __forceinline__ unsigned en_chunks(unsigned n) { return (n + EN_CHUNK - 1u) / EN_CHUNK; }

// Sum and maximum over the workgroup in a fixed order: xor-shuffles over each wave, then (0+1)+(2+3) in the caller.
__device__ __forceinline__ void en_block_reduce(double& sum, unsigned long long& mx, double* red_s, unsigned long long* red_m) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    const unsigned long long other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if ((threadIdx.x & 63u) == 0u) {
    red_s[threadIdx.x >> 6] = sum;
    red_m[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
}
__device__ __forceinline__ double en_total(const double* red_s) {
#pragma clang fp contract(off)
  return (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
}
__device__ __forceinline__ unsigned long long en_max(const unsigned long long* red_m) {
  return std::max(std::max(red_m[0], red_m[1]), std::max(red_m[2], red_m[3]));
}

__global__ __launch_bounds__(EN_THREADS) void ensemble_kernel(EnTable tab, const unsigned char* __restrict__ samples, int K,
                                                              unsigned magic, unsigned char* __restrict__ mean_u8,
                                                              unsigned char* __restrict__ std_u8, float* __restrict__ mean01,
                                                              double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) unsigned char tile[EN_CHUNK];    // the chunk's mean bytes, for the planar mean01 stores
  __shared__ double red_s[4];
  __shared__ unsigned long long red_m[4];
  const EnImage im = tab.im[blockIdx.y];
  const unsigned n = im.n, nchunks = en_chunks(n);
  const long long stride = ((long long)n + (EN_VEC - 1)) & ~(long long)(EN_VEC - 1);
  const unsigned char* src = samples + (long long)EN_VEC * im.in_off16;
  unsigned char* dst_m = mean_u8 + (long long)EN_VEC * im.out_off16;
  unsigned char* dst_s = std_u8 + (long long)EN_VEC * im.out_off16;
  double* part = partials + 2ull * im.part;
  const unsigned long long K2 = (unsigned long long)((unsigned)K * (unsigned)K);
  const float two_over_k = 2.0f / (float)K;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (unsigned chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const unsigned c0 = chunk * EN_CHUNK;                            // n < 2^31 - 256: no wrap
    const unsigned e0 = c0 + threadIdx.x * EN_VEC;                   // the lane's first element
    const unsigned valid = e0 >= n ? 0u : std::min((unsigned)EN_VEC, n - e0);
    unsigned S[EN_VEC], Q[EN_VEC];
#pragma unroll
    for (int j = 0; j < EN_VEC; ++j) S[j] = Q[j] = 0u;
    if (valid != 0u) {
      const unsigned char* p = src + e0;
#pragma unroll 2
      for (int k = 0; k < K; ++k, p += stride) {
        unsigned wd[4] = {0u, 0u, 0u, 0u};
        if (valid == (unsigned)EN_VEC) {
          const uint4 v = *reinterpret_cast<const uint4*>(p);
          wd[0] = v.x, wd[1] = v.y, wd[2] = v.z, wd[3] = v.w;
        } else {                                                     // the image's last, partial vector: byte by byte
#pragma unroll
          for (int j = 0; j < EN_VEC; ++j)
            if ((unsigned)j < valid) wd[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
        }
#pragma unroll
        for (int j = 0; j < EN_VEC; ++j) {
          const unsigned x = (wd[j >> 2] >> (8 * (j & 3))) & 0xffu;
          S[j] += x;
          Q[j] += x * x;
        }
      }
    }
    unsigned mw[4] = {0u, 0u, 0u, 0u}, sw[4] = {0u, 0u, 0u, 0u};
    double sum = 0.0;
    unsigned long long mx = 0ull;
#pragma unroll
    for (int j = 0; j < EN_VEC; ++j) {                               // an element past the end has S = Q = 0: m = s = D = 0
      const unsigned long long D = (unsigned long long)(unsigned)K * Q[j] - (unsigned long long)S[j] * S[j];
      const unsigned m = __umulhi(2u * S[j] + (unsigned)K, magic);
      // 2 sigma in fp32 is within 1e-3 of its value (sqrtf and the product: a few ulp of at most 255), so the estimate is the
      // rounded value or its neighbour; the integer comparison settles which
      unsigned s = (unsigned)(sqrtf((float)(unsigned)D) * two_over_k + 0.5f);
      s = std::min(s, 255u);
      const unsigned long long D16 = 16ull * D;
      const unsigned up = 2u * s + 1u, dn = 2u * s - 1u;
      if ((unsigned long long)(up * up) * K2 <= D16) ++s;
      else if (s > 0u && (unsigned long long)(dn * dn) * K2 > D16) --s;
      mw[j >> 2] |= m << (8 * (j & 3));
      sw[j >> 2] |= s << (8 * (j & 3));
      sum += sqrt((double)D);
      mx = D > mx ? D : mx;
    }
    if (valid == (unsigned)EN_VEC) {
      *reinterpret_cast<uint4*>(dst_m + e0) = make_uint4(mw[0], mw[1], mw[2], mw[3]);
      *reinterpret_cast<uint4*>(dst_s + e0) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
    } else {
#pragma unroll
      for (int j = 0; j < EN_VEC; ++j) {
        if ((unsigned)j < valid) {
          dst_m[e0 + j] = (unsigned char)((mw[j >> 2] >> (8 * (j & 3))) & 0xffu);
          dst_s[e0 + j] = (unsigned char)((sw[j >> 2] >> (8 * (j & 3))) & 0xffu);
        }
      }
    }
    if (mean01 != nullptr) {                                         // the same in every thread of the launch
      *reinterpret_cast<uint4*>(tile + threadIdx.x * EN_VEC) = make_uint4(mw[0], mw[1], mw[2], mw[3]);
      __syncthreads();
      const unsigned hw = n / 3u;
      const unsigned wb = c0 + wave * EN_WAVE;                       // the wave's elements: [wb, we)
      if (wb < n) {
        const unsigned we = std::min(wb + EN_WAVE, n);
        float* o = mean01 + im.m01_off;
#pragma unroll
        for (unsigned c = 0; c < 3u; ++c) {                          // pixels p with wb <= 3 p + c < we
          const unsigned p_lo = (wb + 2u - c) / 3u, p_hi = (we + 2u - c) / 3u;
          for (unsigned p = p_lo + lane; p < p_hi; p += 64u)
            o[(size_t)c * hw + p] = (float)tile[3u * p + c - c0] / 255.0f;
        }
      }
    }
    en_block_reduce(sum, mx, red_s, red_m);
    if (threadIdx.x == 0u) {
      part[2ull * chunk] = en_total(red_s);
      part[2ull * chunk + 1] = __longlong_as_double((long long)en_max(red_m));
    }
    __syncthreads();                                                 // red and tile are written again in the next pass
  }
}

// One workgroup per image: the image's records combined in a fixed order, then the two numbers.
__global__ __launch_bounds__(EN_THREADS) void ensemble_finish_kernel(EnTable tab, int K, const double* __restrict__ partials,
                                                                     double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double red_s[4];
  __shared__ unsigned long long red_m[4];
  const EnImage im = tab.im[blockIdx.x];
  const unsigned nchunks = en_chunks(im.n);
  const double* part = partials + 2ull * im.part;
  double sum = 0.0;
  unsigned long long mx = 0ull;
  for (unsigned k = threadIdx.x; k < nchunks; k += EN_THREADS) {
    sum += part[2ull * k];
    const unsigned long long d = (unsigned long long)__double_as_longlong(part[2ull * k + 1]);
    mx = d > mx ? d : mx;
  }
  en_block_reduce(sum, mx, red_s, red_m);
  if (threadIdx.x == 0u) {
    double* res = stats + 2ull * blockIdx.x;
    res[0] = (en_total(red_s) / (double)K) / (double)im.n;
    res[1] = sqrt((double)en_max(red_m)) / (double)K;
  }
}

int ensemble_images(const char* who, const uint8_t* samples, const int64_t* sample_offsets, const int32_t* hw, int n_images, int K,
                    uint8_t* mean_u8, uint8_t* std_u8, const int64_t* out_offsets, float* mean01, const int64_t* m01_offsets,
                    double* stats, double* scratch, hipStream_t st) {
  const std::string name(who);
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!samples || !sample_offsets || !hw || !mean_u8 || !std_u8 || !out_offsets || !stats || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if ((mean01 == nullptr) != (m01_offsets == nullptr)) SRGD_EXT_FAIL(name + ": mean01 and its offsets are given together or not at all");
  if (K < 2 || K > 256) SRGD_EXT_FAIL(name + ": n_samples must be in 2..256");
  if ((((uintptr_t)samples | (uintptr_t)mean_u8 | (uintptr_t)std_u8) & (uintptr_t)(EN_VEC - 1)) != 0)
    SRGD_EXT_FAIL(name + ": samples, mean_u8 and std_u8 must be 16-byte aligned");
  if ((((uintptr_t)stats | (uintptr_t)scratch) & 7u) != 0 || ((uintptr_t)mean01 & 3u) != 0)
    SRGD_EXT_FAIL(name + ": stats and scratch must be 8-byte aligned, mean01 4-byte aligned");
  unsigned long long total = 0;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const long long h = hw[2 * i], w = hw[2 * i + 1];
    if (h < 1 || w < 1) SRGD_EXT_FAIL(name + ": bad size");
    if (3 * h * w >= 0x7fffff00ll) SRGD_EXT_FAIL(name + ": image of 2^31 - 256 elements or more");
    for (const int64_t off : {sample_offsets[i], out_offsets[i]}) {
      if (off < 0 || off >= (1ll << 36)) SRGD_EXT_FAIL(name + ": offset outside [0, 2^36)");
      if ((off & (EN_VEC - 1)) != 0) SRGD_EXT_FAIL(name + ": misaligned offset (sample and output offsets are multiples of 16)");
    }
    if (m01_offsets && m01_offsets[i] < 0) SRGD_EXT_FAIL(name + ": negative mean01 offset");
    total += (unsigned long long)((3 * h * w + EN_CHUNK - 1) / EN_CHUNK);
  }
  if (total > 0xffffffffull) SRGD_EXT_FAIL(name + ": more than 2^32 chunks in one call");
  const unsigned magic = (unsigned)((1ull << 32) / (unsigned)(2 * K)) + 1u;
  unsigned part = 0;                                     // records, packed in image order
  for (int first = 0; first < n_images; first += EN_MAX_IMAGES) {     // one launch sequence per EN_MAX_IMAGES images
    const int cnt = std::min(EN_MAX_IMAGES, n_images - first);
    EnTable tab;
    unsigned max_chunks = 0;
    for (int k = 0; k < EN_MAX_IMAGES; ++k) tab.im[k] = EnImage{0, 0u, 0u, 0u, 0u};
    for (int k = 0; k < cnt; ++k) {
      const int i = first + k;
      const unsigned n = 3u * (unsigned)hw[2 * i] * (unsigned)hw[2 * i + 1];
      const unsigned chunks = (n + EN_CHUNK - 1u) / EN_CHUNK;
      tab.im[k] = EnImage{m01_offsets ? (long long)m01_offsets[i] : 0ll, (unsigned)(sample_offsets[i] / EN_VEC),
                          (unsigned)(out_offsets[i] / EN_VEC), n, part};
      part += chunks;
      max_chunks = std::max(max_chunks, chunks);
    }
    hipLaunchKernelGGL(ensemble_kernel, dim3(std::min(max_chunks, EN_MAX_GRID_X), (unsigned)cnt), dim3(EN_THREADS), 0, st, tab, samples,
                       K, magic, mean_u8, std_u8, mean01, scratch);
    hipLaunchKernelGGL(ensemble_finish_kernel, dim3((unsigned)cnt), dim3(EN_THREADS), 0, st, tab, K, scratch, stats + (size_t)first * 2);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_image_ensemble_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_image_ensemble(const uint8_t* samples, int n_samples, int h, int w, uint8_t* mean_u8, uint8_t* std_u8, float* mean01,
                                        double* stats, double* scratch, void* stream) {
  const int64_t off = 0;
  const int32_t hw[2] = {h, w};
  return ensemble_images("srgd_image_ensemble", samples, &off, hw, 1, n_samples, mean_u8, std_u8, &off, mean01, mean01 ? &off : nullptr,
                         stats, scratch, (hipStream_t)stream);
}

SRGD_EXT_EXPORT int srgd_image_ensemble_images(const uint8_t* samples, const int64_t* sample_offsets_host, const int32_t* hw_host, int n_images,
                                               int n_samples, uint8_t* mean_u8, uint8_t* std_u8, const int64_t* out_offsets_host,
                                               float* mean01, const int64_t* mean01_offsets_host, double* stats, double* scratch,
                                               void* stream) {
  return ensemble_images("srgd_image_ensemble_images", samples, sample_offsets_host, hw_host, n_images, n_samples, mean_u8, std_u8,
                         out_offsets_host, mean01, mean01_offsets_host, stats, scratch, (hipStream_t)stream);
}

}  // extern "C"
