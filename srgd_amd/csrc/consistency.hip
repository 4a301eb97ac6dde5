// LR consistency of a x4 super-resolved image on the GPU (engine extension, absent upstream): the output AS SAVED is reduced by 4
// with the operator that made the condition - Pillow's Image.resize(BICUBIC) - and compared with the low-resolution input it was
// sampled from.  Inputs and outputs are 8-bit, so every result is an exact integer; the definition is fixed in
// include/srgd_consistency.h and restated here in short.
//
// Definition, per image: L uint8 [h][w][3], O uint8 [4h][4w][3], D = Image.resize((w, h), BICUBIC) of O as Pillow's
// src/libImaging/Resample.c computes it (coefficients of precompute_coeffs: support 8, a = -0.5, window clipped to the image and
// renormalised, 22-bit fixed point, round half away from zero; horizontal pass over all 4h rows, accumulator 1 << 21, clip8(acc >> 22),
// rounded to 8 bits; then the vertical pass on that result); e = D - L; sse_r, sse_g, sse_b = sum e^2 per channel, max_abs = max |e|.
//
// The window facts.  For n >= 5 outputs of 4n inputs, output i in 2 .. n-3 reads the 16 inputs from 4i - 6 with one symmetric
// vector; outputs 0, 1, n-2, n-1 read 10, 14, 14, 10 inputs of the clipped window with vectors of their own; none depends on n.
// Here every vector is laid on the frame [4i - 6, 4i + 10) of its output with zeros on the taps outside the image, so one loop
// of 16 taps serves every output, and the inputs outside the image are staged as zeros.  The five vectors (320 bytes) are computed
// once on the host by Pillow's formula and travel as a kernel argument.
//
// Work split.  One workgroup of 256 threads per tile of 32 x 15 LR pixels (width x height); blockIdx.y is the image (its record
// travels in the kernel argument), blockIdx.x the tile.
//   1. The HR patch of the tile - 72 rows (60 + a halo of 6 on each side) of 448 bytes: the 420 bytes of 140 pixels, begun 14
//      bytes early so that a patch row starts on a 16-byte boundary of the image row - goes to LDS, one 16-byte load per lane where
//      the image rows are 16-byte aligned (12 w bytes per row: w % 4 == 0) and the vector lies inside the row, four guarded 4-byte
//      loads otherwise (12 w is a multiple of 4: a dword never straddles a row's end).  Bytes outside the image are zeros.
//   2. Horizontal pass, LDS to LDS as uint8 - the rounding Pillow does between the passes: a thread owns one LR column of the tile
//      (its 16 coefficients stay in registers) and takes 9 of the 72 patch rows; per row it reads the 13 dwords that hold the 48
//      bytes of its window and writes 3 bytes.
//   3. Vertical pass: a thread takes 4 consecutive bytes of an LR row of the tile (one dword of each of 16 rows of the h-pass result),
//   4. subtracts L, stores D where asked (byte stores under the guard of the image's size), and the squares per channel and the
//      maximum are reduced over the workgroup in integers: one record {sse_r, sse_g, sse_b, max_abs} of 4 x 8 bytes per tile,
//      stored plainly.
// A second kernel, one workgroup per image, adds the records.  No atomics; sums of integers: an image's D and its four integers are
// bit-identical alone, in any group and at any offset.
// LDS: 32,256 (patch) + 6,912 (h-pass) + 320 (coefficients) + 64 (reduction) = 39,552 bytes: four workgroups per CU.  HR bytes read
// per HR byte owned: 72/60 * 448/384 = 1.40.
// Accumulators are int32 as Pillow's (255 * sum |k| ~ 1.3e9 < 2^31); every |k| < 2^23, so a tap is one 24-bit multiply-add.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_consistency.h"
#include "pillow_x4.hpp"

// This file is a library of its own (libsrgd_consistency.so, include/srgd_consistency.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing, pillow_x4.hpp the selectors of the x4 vectors and the byte extractor it
// has in common with backproject.hip and guidance.hip.
namespace srgd {
namespace {

constexpr int CS_TAPS = 16;
constexpr int CS_THREADS = 256;
constexpr int CS_TW = 32, CS_TH = 15;                // LR pixels of a tile
constexpr int CS_PROWS = 4 * CS_TH + 12;             // HR rows of the patch: 72
constexpr int CS_PVEC = 28;                          // 16-byte vectors of a patch row: bytes [12 tx0 - 32, 12 tx0 + 416) of the image row
constexpr int CS_PSTRIDE = 16 * CS_PVEC;             // 448
constexpr int CS_HSTRIDE = 3 * CS_TW;                // bytes of a row of the h-pass result: 96
constexpr int CS_HDWORDS = CS_HSTRIDE / 4;           // 24
constexpr int CS_MAX_IMAGES = 128;                   // records travel as a kernel argument (3 KiB)
static_assert(CS_PROWS % (CS_THREADS / CS_TW) == 0, "the h-pass gives every thread the same number of rows");
static_assert(12 * (CS_TW - 1) + 12 + 52 <= CS_PSTRIDE, "the 13 dwords of the last column lie inside the patch row");

struct CsImage {
  unsigned hr_off16, lr_off16, down_off16;           // first byte of O, L, D in units of 16 bytes
  int h, w;                                          // LR size
  unsigned part;                                     // first record of the image in the scratch
};
struct CsTable { CsImage im[CS_MAX_IMAGES]; };
struct CsCoeffs { int k[5][CS_TAPS]; };              // row 0, row 1, interior, row n-2, row n-1, each on the frame [4i - 6, 4i + 10)
struct CsRecord { unsigned long long sse[3], max_abs; };

__host__ __device__ inline unsigned cs_tiles_x(int w) { return (unsigned)((w + CS_TW - 1) / CS_TW); }
__host__ __device__ inline unsigned cs_tiles_y(int h) { return (unsigned)((h + CS_TH - 1) / CS_TH); }

__global__ __launch_bounds__(CS_THREADS) void consistency_tile_kernel(CsTable tab, CsCoeffs coeffs, const unsigned char* __restrict__ hr_u8,
                                                                      const unsigned char* __restrict__ lr_u8,
                                                                      unsigned char* __restrict__ down_u8, CsRecord* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) unsigned char patch[CS_PROWS * CS_PSTRIDE];
  __shared__ __attribute__((aligned(16))) unsigned char hbuf[CS_PROWS * CS_HSTRIDE];
  __shared__ __attribute__((aligned(16))) int kk[5][CS_TAPS];
  __shared__ unsigned red[4][4];
  const CsImage im = tab.im[blockIdx.y];
  const int h = im.h, w = im.w;
  const unsigned tiles_x = cs_tiles_x(w);
  if (blockIdx.x >= tiles_x * cs_tiles_y(h)) return;                 // the grid is as wide as the launch's largest image
  const int tx0 = (int)(blockIdx.x % tiles_x) * CS_TW, ty0 = (int)(blockIdx.x / tiles_x) * CS_TH;
  const int tid = (int)threadIdx.x;
  if (tid < 5 * CS_TAPS) kk[tid >> 4][tid & 15] = coeffs.k[tid >> 4][tid & 15];

  // 1. the HR patch: patch row r is image row 4 ty0 - 6 + r, patch byte q of it is byte 12 tx0 - 32 + q of that image row
  const int row_bytes = 12 * w;                                      // 3 * 4w
  const unsigned char* src = hr_u8 + 16ull * im.hr_off16;
  const bool rows_aligned = (w & 3) == 0;
  for (int i = tid; i < CS_PROWS * CS_PVEC; i += CS_THREADS) {
    const int r = i / CS_PVEC, v = i - r * CS_PVEC;
    const int y = 4 * ty0 - 6 + r, gb = 12 * tx0 - 32 + 16 * v;
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if (y >= 0 && y < 4 * h) {
      const unsigned char* p = src + (size_t)y * (size_t)row_bytes + gb;      // read only where the guards below hold
      if (rows_aligned && gb >= 0 && gb + 16 <= row_bytes) {
        val = *reinterpret_cast<const uint4*>(p);
      } else {
        if (gb >= 0 && gb + 4 <= row_bytes) val.x = *reinterpret_cast<const unsigned*>(p);
        if (gb + 4 >= 0 && gb + 8 <= row_bytes) val.y = *reinterpret_cast<const unsigned*>(p + 4);
        if (gb + 8 >= 0 && gb + 12 <= row_bytes) val.z = *reinterpret_cast<const unsigned*>(p + 8);
        if (gb + 12 >= 0 && gb + 16 <= row_bytes) val.w = *reinterpret_cast<const unsigned*>(p + 12);
      }
    }
    *reinterpret_cast<uint4*>(patch + r * CS_PSTRIDE + 16 * v) = val;
  }
  __syncthreads();

  // 2. horizontal pass: column x of the tile, rows tid / 32 + 8 it.  The window of output tx0 + x begins at image byte
  //    12 (tx0 + x) - 18 = patch byte 12 x + 14: the 13 dwords from patch byte 12 x + 12 hold it from their byte 2 on.
  {
    const int x = tid & (CS_TW - 1);
    int kx[CS_TAPS];
    const int4* kv = reinterpret_cast<const int4*>(kk[x4_down_vector(tx0 + x, w)]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 c = kv[q];
      kx[4 * q] = c.x, kx[4 * q + 1] = c.y, kx[4 * q + 2] = c.z, kx[4 * q + 3] = c.w;
    }
    for (int r = tid / CS_TW; r < CS_PROWS; r += CS_THREADS / CS_TW) {
      const unsigned* p = reinterpret_cast<const unsigned*>(patch + r * CS_PSTRIDE + 12 * x + 12);
      unsigned d[13];
#pragma unroll
      for (int q = 0; q < 13; ++q) d[q] = p[q];
      int acc[3] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
#pragma unroll
      for (int t = 0; t < CS_TAPS; ++t) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += __mul24(kx[t], u8_of(d, 2 + 3 * t + c));
      }
      unsigned char* o = hbuf + r * CS_HSTRIDE + 3 * x;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (unsigned char)clip8(acc[c]);
    }
  }
  __syncthreads();

  // 3. + 4. vertical pass on the rounded bytes: an item is dword j of LR row yl of the tile = elements 4 j .. 4 j + 3 of that row
  unsigned sse[3] = {0u, 0u, 0u}, mx = 0u;
  const unsigned char* lr = lr_u8 + 16ull * im.lr_off16;
  unsigned char* down = down_u8 != nullptr ? down_u8 + 16ull * im.down_off16 : nullptr;
  for (int i = tid; i < CS_TH * CS_HDWORDS; i += CS_THREADS) {
    const int yl = i / CS_HDWORDS, j = i - yl * CS_HDWORDS;
    const int gy = ty0 + yl;
    if (gy >= h) continue;
    const int4* kv = reinterpret_cast<const int4*>(kk[x4_down_vector(gy, h)]);
    int ky[CS_TAPS];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 c = kv[q];
      ky[4 * q] = c.x, ky[4 * q + 1] = c.y, ky[4 * q + 2] = c.z, ky[4 * q + 3] = c.w;
    }
    int acc[4] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
    const unsigned* p = reinterpret_cast<const unsigned*>(hbuf + 4 * yl * CS_HSTRIDE) + j;
#pragma unroll
    for (int t = 0; t < CS_TAPS; ++t) {
      const unsigned d = p[t * CS_HDWORDS];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] += __mul24(ky[t], u8_of(&d, b));
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int e = 4 * j + b, px = e / 3, c = e - 3 * px;
      const int gx = tx0 + px;
      if (gx < w) {
        const unsigned g = ((unsigned)gy * (unsigned)w + (unsigned)gx) * 3u + (unsigned)c;      // < 2^31 / 16
        const int dv = clip8(acc[b]);
        if (down != nullptr) down[g] = (unsigned char)dv;
        const int err = dv - (int)lr[g];
        const unsigned a = (unsigned)(err < 0 ? -err : err), sq = a * a;
        sse[0] += c == 0 ? sq : 0u;
        sse[1] += c == 1 ? sq : 0u;
        sse[2] += c == 2 ? sq : 0u;
        mx = a > mx ? a : mx;
      }
    }
  }
  // a thread holds at most 8 squares of at most 255^2, a tile 1,440: 32 bits hold the tile's sums; the record is 64-bit
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sse[0] += __shfl_xor(sse[0], o, 64);
    sse[1] += __shfl_xor(sse[1], o, 64);
    sse[2] += __shfl_xor(sse[2], o, 64);
    const unsigned other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = sse[0], red[tid >> 6][1] = sse[1], red[tid >> 6][2] = sse[2], red[tid >> 6][3] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    CsRecord rec;
#pragma unroll
    for (int c = 0; c < 3; ++c) rec.sse[c] = (unsigned long long)red[0][c] + red[1][c] + red[2][c] + red[3][c];
    rec.max_abs = std::max(std::max(red[0][3], red[1][3]), std::max(red[2][3], red[3][3]));
    partials[(size_t)im.part + blockIdx.x] = rec;
  }
}

// One workgroup per image: the image's tile records added (integers: any order gives the same sums), then the four int64.
__global__ __launch_bounds__(CS_THREADS) void consistency_finish_kernel(CsTable tab, const CsRecord* __restrict__ partials,
                                                                        long long* __restrict__ stats) {
  __shared__ unsigned long long red[4][4];
  const CsImage im = tab.im[blockIdx.x];
  const unsigned ntiles = cs_tiles_x(im.w) * cs_tiles_y(im.h);
  const CsRecord* part = partials + im.part;
  unsigned long long s[3] = {0ull, 0ull, 0ull}, mx = 0ull;
  for (unsigned k = threadIdx.x; k < ntiles; k += CS_THREADS) {
    const CsRecord rec = part[k];
    s[0] += rec.sse[0], s[1] += rec.sse[1], s[2] += rec.sse[2];
    mx = rec.max_abs > mx ? rec.max_abs : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s[0] += __shfl_xor(s[0], o, 64);
    s[1] += __shfl_xor(s[1], o, 64);
    s[2] += __shfl_xor(s[2], o, 64);
    const unsigned long long other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if ((threadIdx.x & 63u) == 0u) {
    red[threadIdx.x >> 6][0] = s[0], red[threadIdx.x >> 6][1] = s[1], red[threadIdx.x >> 6][2] = s[2], red[threadIdx.x >> 6][3] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    long long* res = stats + 4ull * blockIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c] = (long long)(red[0][c] + red[1][c] + red[2][c] + red[3][c]);
    res[3] = (long long)std::max(std::max(red[0][3], red[1][3]), std::max(red[2][3], red[3][3]));
  }
}

int consistency_images(const char* who, const uint8_t* hr_u8, const int64_t* hr_offsets, const uint8_t* lr_u8, const int64_t* lr_offsets,
                       const int32_t* hw, int n_images, uint8_t* down_u8, const int64_t* down_offsets, int64_t* stats, void* scratch,
                       hipStream_t st) {
  const std::string name(who);
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!hr_u8 || !hr_offsets || !lr_u8 || !lr_offsets || !hw || !stats || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if ((down_u8 == nullptr) != (down_offsets == nullptr)) SRGD_EXT_FAIL(name + ": down_u8 and its offsets are given together or not at all");
  if (((uintptr_t)hr_u8 & 15u) != 0) SRGD_EXT_FAIL(name + ": hr_u8 must be 16-byte aligned");
  if ((((uintptr_t)stats | (uintptr_t)scratch) & 7u) != 0) SRGD_EXT_FAIL(name + ": stats and scratch must be 8-byte aligned");
  unsigned long long total = 0;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const long long h = hw[2 * i], w = hw[2 * i + 1];
    if (h < 5 || w < 5) SRGD_EXT_FAIL(name + ": bad size (h and w must be >= 5: smaller windows overlap and depend on the size)");
    if (48 * h * w >= 0x7fffff00ll) SRGD_EXT_FAIL(name + ": output of 2^31 - 256 elements or more");
    for (const int64_t off : {hr_offsets[i], lr_offsets[i], down_offsets ? down_offsets[i] : (int64_t)0}) {
      if (off < 0 || off >= (1ll << 36)) SRGD_EXT_FAIL(name + ": offset outside [0, 2^36)");
      if ((off & 15) != 0) SRGD_EXT_FAIL(name + ": misaligned offset (offsets are multiples of 16)");
    }
    total += (unsigned long long)cs_tiles_x((int)w) * cs_tiles_y((int)h);
  }
  if (total > 0xffffffffull) SRGD_EXT_FAIL(name + ": more than 2^32 tiles in one call");
  static const CsCoeffs coeffs = [] {                    // pillow_coeffs.hpp: the five vectors on the frames of their outputs
    CsCoeffs c;
    pillow::x4_reduce_vectors(c.k, true);
    return c;
  }();
  unsigned part = 0;                                     // records, packed in image order
  for (int first = 0; first < n_images; first += CS_MAX_IMAGES) {     // one launch sequence per CS_MAX_IMAGES images
    const int cnt = std::min(CS_MAX_IMAGES, n_images - first);
    CsTable tab;
    unsigned max_tiles = 0;
    for (int k = 0; k < CS_MAX_IMAGES; ++k) tab.im[k] = CsImage{0u, 0u, 0u, 0, 0, 0u};
    for (int k = 0; k < cnt; ++k) {
      const int i = first + k;
      const unsigned tiles = cs_tiles_x(hw[2 * i + 1]) * cs_tiles_y(hw[2 * i]);
      tab.im[k] = CsImage{(unsigned)(hr_offsets[i] / 16), (unsigned)(lr_offsets[i] / 16),
                          down_offsets ? (unsigned)(down_offsets[i] / 16) : 0u, hw[2 * i], hw[2 * i + 1], part};
      part += tiles;
      max_tiles = std::max(max_tiles, tiles);
    }
    hipLaunchKernelGGL(consistency_tile_kernel, dim3(max_tiles, (unsigned)cnt), dim3(CS_THREADS), 0, st, tab, coeffs, hr_u8, lr_u8,
                       down_u8, (CsRecord*)scratch);
    hipLaunchKernelGGL(consistency_finish_kernel, dim3((unsigned)cnt), dim3(CS_THREADS), 0, st, tab, (const CsRecord*)scratch,
                       (long long*)stats + (size_t)first * 4);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_image_consistency_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_image_consistency_coeffs(int32_t out[5][16]) {
  if (!out) SRGD_EXT_FAIL("srgd_image_consistency_coeffs: null argument");
  pillow::x4_reduce_vectors(out, false);
  return 0;
}

SRGD_EXT_EXPORT int srgd_image_consistency(const uint8_t* hr_u8, const uint8_t* lr_u8, int h, int w, uint8_t* down_u8, int64_t* stats,
                                           void* scratch, void* stream) {
  const int64_t off = 0;
  const int32_t hw[2] = {h, w};
  return consistency_images("srgd_image_consistency", hr_u8, &off, lr_u8, &off, hw, 1, down_u8, down_u8 ? &off : nullptr, stats, scratch,
                            (hipStream_t)stream);
}

SRGD_EXT_EXPORT int srgd_image_consistency_images(const uint8_t* hr_u8, const int64_t* hr_offsets_host, const uint8_t* lr_u8,
                                                  const int64_t* lr_offsets_host, const int32_t* hw_host, int n_images, uint8_t* down_u8,
                                                  const int64_t* down_offsets_host, int64_t* stats, void* scratch, void* stream) {
  return consistency_images("srgd_image_consistency_images", hr_u8, hr_offsets_host, lr_u8, lr_offsets_host, hw_host, n_images, down_u8,
                            down_offsets_host, stats, scratch, (hipStream_t)stream);
}

}  // extern "C"
