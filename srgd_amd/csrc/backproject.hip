// Iterative back-projection of a x4 super-resolved image onto its own low-resolution input on the GPU (engine extension, absent
// upstream): O <- clip(O + C - enlarge(reduce(O))), N times, with the two operators the project owns as Pillow-exact integer code -
// the x4 reduction of consistency.hip and the x4 enlargement of imageio.hip.  Everything between the two quantisations is 8-bit, so
// every result is an exact integer; the definition is fixed in include/srgd_backproject.h and restated here in short.
//
// Definition, per image: out01, cond01 fp32 planar [3][H][W], H = 4h, W = 4w.  O_0 = q(out01) (mul 255, truncate, saturate, NaN -> 0),
// C = r(cond01) (mul 255, round half up, saturate, NaN -> 0), both uint8 [H][W][3].  For k = 1 .. N: D = Image.resize((w, h), BICUBIC)
// of O_{k-1}, U = Image.resize((W, H), BICUBIC) of D, both as Pillow's src/libImaging/Resample.c computes them (22-bit fixed point,
// horizontal pass rounded to 8 bits, then the vertical pass), O_k = clip(O_{k-1} + C - U, 0, 255).  dst01 = O_N / 255, planar; where
// out01 was non-finite, dst01 is out01.
//
// The window facts.  Reduction (4n -> n, n >= 5): output i in 2 .. n-3 reads the 16 inputs from 4i - 6 with one symmetric vector;
// outputs 0, 1, n-2, n-1 read 10, 14, 14, 10 inputs of the clipped window with vectors of their own.  Enlargement (n -> 4n): output j
// in 6 .. 4n-7 reads the 4 inputs from (j - 6) / 4 with the vector of its phase (j - 6) % 4; outputs 0 .. 5 read 2, 2, 3, 3, 3, 3
// inputs from 0 and outputs 4n-6 .. 4n-1 read 3, 3, 3, 3, 2, 2 inputs that end at n-1, with vectors of their own.  No vector depends
// on n.  Here every vector is laid on the frame of its output - [4i - 6, 4i + 10) for the reduction, [floor((j - 6) / 4),
// floor((j - 6) / 4) + 4) for the enlargement - with zeros on the taps outside the image, so one loop of 16 (of 4) taps serves every
// output, and the inputs outside the image are staged as zeros.  The vectors are computed once on the host by Pillow's formula and
// travel as kernel arguments.
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument).
//   begin:  a thread takes 4 consecutive pixels: 4 floats of each of the 3 planes of out01 and of cond01 (one 16-byte load each where
//           the plane is 16-byte aligned) become 12 bytes of O and 12 bytes of C (3 dword stores each).
//   reduce: one workgroup of 256 threads per tile of 32 x 15 LR pixels, the tiling and the passes of consistency.hip's tile kernel:
//           the HR patch of the tile (72 rows of 448 bytes) goes to LDS, horizontal pass LDS to LDS as uint8, vertical pass, D stored.
//   update: one workgroup per tile of 128 x 60 HR pixels = the same 32 x 15 LR pixels.  The tile's D rows and columns plus a halo of
//           2 (19 rows x 36 pixels, zeros outside the image) go to LDS; horizontal pass to 19 rows x 384 bytes in LDS: a thread owns
//           one HR column (its 4 coefficients stay in registers) and takes every second row; vertical pass and correction: a thread
//           takes one dword of an HR row (4 bytes of U from one dword of each of 4 rows of the h-pass result), reads that dword of O
//           and of C and writes O in place - a workgroup reads O only at the elements it writes.  Rows of O are 12 w bytes and a tile
//           row begins at byte 384 * tile: every dword is aligned and lies inside the row or outside it.
//   end:    the mirror image of begin: 12 bytes of O and 4 floats of each plane of out01 become 4 floats of each plane of dst01.
// No atomics, no reductions: every byte depends on the image's own bytes alone - bit-identical alone, in any group, at any offset.
// LDS: reduce 32,256 (patch) + 6,912 (h-pass) + 320 (coefficients) = 39,488 bytes; update 2,128 + 7,296 + 256 = 9,680 bytes.
// Bytes moved per iteration and LR pixel: reduce reads 48 * 1.40 and writes 3; update reads 48 (O) + 48 (C) + 3 * 1.43 (D, with the
// halo) and writes 48.
// Accumulators are int32 as Pillow's; every |k| < 2^23, so a tap is one 24-bit multiply-add.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_backproject.h"
#include "pillow_x4.hpp"

// This file is a library of its own (libsrgd_backproject.so, include/srgd_backproject.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing, pillow_x4.hpp the selectors of the x4 vectors and the byte extractor it
// has in common with consistency.hip and guidance.hip.
namespace srgd {
namespace {

constexpr int BP_THREADS = 256;
constexpr int BP_TW = 32, BP_TH = 15;                // LR pixels of a tile
constexpr int BP_MAX_IMAGES = 128;                   // records travel as a kernel argument (3 KiB)
constexpr int BP_MAX_ITERATIONS = 64;
// reduce
constexpr int BP_RTAPS = 16;
constexpr int BP_PROWS = 4 * BP_TH + 12;             // HR rows of the patch: 72
constexpr int BP_PVEC = 28;                          // 16-byte vectors of a patch row: bytes [12 tx0 - 32, 12 tx0 + 416) of the image row
constexpr int BP_PSTRIDE = 16 * BP_PVEC;             // 448
constexpr int BP_HSTRIDE = 3 * BP_TW;                // bytes of a row of the reduction's h-pass result: 96
constexpr int BP_HDWORDS = BP_HSTRIDE / 4;           // 24
static_assert(BP_PROWS % (BP_THREADS / BP_TW) == 0, "the h-pass gives every thread the same number of rows");
static_assert(12 * (BP_TW - 1) + 12 + 52 <= BP_PSTRIDE, "the 13 dwords of the last column lie inside the patch row");
// update
constexpr int BP_UTAPS = 4;
constexpr int BP_UW = 4 * BP_TW, BP_UH = 4 * BP_TH;  // HR pixels of a tile: 128 x 60
constexpr int BP_DROWS = BP_TH + 4;                  // LR rows of the D patch: 19 (rows ty0 - 2 .. ty0 + 16)
constexpr int BP_DCOLS = BP_TW + 4;                  // LR pixels of a D patch row: 36 (columns tx0 - 2 .. tx0 + 33)
constexpr int BP_DBYTES = 3 * BP_DCOLS;              // 108
constexpr int BP_DSTRIDE = 112;                      // ... in a row of whole dwords
constexpr int BP_USTRIDE = 3 * BP_UW;                // bytes of a row of the enlargement's h-pass result: 384
constexpr int BP_UDWORDS = BP_USTRIDE / 4;           // 96
static_assert(BP_THREADS == 2 * BP_UW, "the enlargement's h-pass: a thread per HR column, two rows at a time");
static_assert((3 * ((BP_UW - 1 + 2) >> 2) & ~3) + 16 <= BP_DSTRIDE, "the 4 dwords of the last column lie inside the D patch row");
static_assert(((BP_UH - 1 + 2) >> 2) + BP_UTAPS <= BP_DROWS, "the 4 rows of the last HR row lie inside the D patch");

struct BpImage {
  long long off;                                     // first element of the image's planes in out01, cond01, dst01
  unsigned long long scr;                            // first byte of the image's scratch (a multiple of 256)
  int h, w;                                          // LR size
};
struct BpTable { BpImage im[BP_MAX_IMAGES]; };
struct BpDown { int k[5][BP_RTAPS]; };               // row 0, row 1, interior, row n-2, row n-1, each on the frame [4i - 6, 4i + 10)
struct BpUp { int k[16][BP_UTAPS]; };                // indices 0 .. 5, phases 0 .. 3, indices 4n-6 .. 4n-1, each on the frame of its output

__host__ __device__ inline unsigned bp_tiles_x(int w) { return (unsigned)((w + BP_TW - 1) / BP_TW); }
__host__ __device__ inline unsigned bp_tiles_y(int h) { return (unsigned)((h + BP_TH - 1) / BP_TH); }
// the image's scratch: O at 0, C at bp_plane(h, w), D at 2 bp_plane(h, w)
__host__ __device__ inline unsigned long long bp_plane(int h, int w) { return round_up(48ull * (unsigned)h * (unsigned)w, 256ull); }
__host__ __device__ inline unsigned long long bp_scratch(int h, int w) {
  return 2ull * bp_plane(h, w) + round_up(3ull * (unsigned)h * (unsigned)w, 256ull);
}

// q: the output as saved (mul 255, truncation), saturated outside [0,1]; NaN -> 0
__device__ __forceinline__ unsigned bp_quant_out(float v) {
  const float t = __fmul_rn(v, 255.0f);
  return !(t > 0.0f) ? 0u : (t >= 255.0f ? 255u : (unsigned)(int)t);
}
// r: the condition rounded to the nearest byte (u8 / 255 -> that u8); NaN -> 0
__device__ __forceinline__ unsigned bp_quant_cond(float v) {
  const float f = floorf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f));
  return !(f > 0.0f) ? 0u : (f >= 255.0f ? 255u : (unsigned)(int)f);
}

// 4 floats from element e (a multiple of 4) of a plane; `vec`: the plane is 16-byte aligned
__device__ __forceinline__ void bp_load4(const float* plane, unsigned e, bool vec, float v[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(plane + e);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = plane[e + k];
  }
}

// out01 -> O, cond01 -> C: a thread per 4 pixels.
__global__ __launch_bounds__(BP_THREADS) void backproject_begin_kernel(BpTable tab, const float* __restrict__ out01,
                                                                       const float* __restrict__ cond01,
                                                                       unsigned char* __restrict__ scratch) {
  const BpImage im = tab.im[blockIdx.y];
  const unsigned npix = 16u * (unsigned)im.h * (unsigned)im.w, quads = npix / 4u;      // npix < 2^31 / 3
  const float* src[2] = {out01 + im.off, cond01 + im.off};
  unsigned char* dst[2] = {scratch + im.scr, scratch + im.scr + bp_plane(im.h, im.w)};
  const bool vec[2] = {((uintptr_t)src[0] & 15u) == 0, ((uintptr_t)src[1] & 15u) == 0};  // a plane is a multiple of 64 bytes
  for (unsigned q = blockIdx.x * BP_THREADS + threadIdx.x; q < quads; q += gridDim.x * BP_THREADS) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[3][4];
#pragma unroll
      for (int c = 0; c < 3; ++c) bp_load4(src[s] + (size_t)c * npix, 4u * q, vec[s], v[c]);
      unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int e = 3 * k + c;
          d[e >> 2] |= (s == 0 ? bp_quant_out(v[c][k]) : bp_quant_cond(v[c][k])) << (8 * (e & 3));
        }
      }
      unsigned* o = reinterpret_cast<unsigned*>(dst[s] + 12ull * q);
      o[0] = d[0], o[1] = d[1], o[2] = d[2];
    }
  }
}

// O -> dst01 (= out01 where out01 is not finite): a thread per 4 pixels.  dst01 may be out01: a thread reads only what it writes.
__global__ __launch_bounds__(BP_THREADS) void backproject_end_kernel(BpTable tab, const float* out01, float* dst01,
                                                                     const unsigned char* __restrict__ scratch) {
  const BpImage im = tab.im[blockIdx.y];
  const unsigned npix = 16u * (unsigned)im.h * (unsigned)im.w, quads = npix / 4u;
  const float* src = out01 + im.off;
  float* dst = dst01 + im.off;
  const unsigned char* o_u8 = scratch + im.scr;
  const bool vec_src = ((uintptr_t)src & 15u) == 0, vec_dst = ((uintptr_t)dst & 15u) == 0;
  for (unsigned q = blockIdx.x * BP_THREADS + threadIdx.x; q < quads; q += gridDim.x * BP_THREADS) {
    const unsigned* p = reinterpret_cast<const unsigned*>(o_u8 + 12ull * q);
    const unsigned d[3] = {p[0], p[1], p[2]};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v[4], r[4];
      bp_load4(src + (size_t)c * npix, 4u * q, vec_src, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = isfinite(v[k]) ? __fdiv_rn((float)u8_of(d, 3 * k + c), 255.0f) : v[k];
      float* o = dst + (size_t)c * npix + 4u * q;
      if (vec_dst) {
        *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = r[k];
      }
    }
  }
}

// D = x4 reduction of O: the tile kernel of consistency.hip without the comparison.
__global__ __launch_bounds__(BP_THREADS) void backproject_reduce_kernel(BpTable tab, BpDown coeffs, unsigned char* __restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) unsigned char patch[BP_PROWS * BP_PSTRIDE];
  __shared__ __attribute__((aligned(16))) unsigned char hbuf[BP_PROWS * BP_HSTRIDE];
  __shared__ __attribute__((aligned(16))) int kk[5][BP_RTAPS];
  const BpImage im = tab.im[blockIdx.y];
  const int h = im.h, w = im.w;
  const unsigned tiles_x = bp_tiles_x(w);
  if (blockIdx.x >= tiles_x * bp_tiles_y(h)) return;                 // the grid is as wide as the launch's largest image
  const int tx0 = (int)(blockIdx.x % tiles_x) * BP_TW, ty0 = (int)(blockIdx.x / tiles_x) * BP_TH;
  const int tid = (int)threadIdx.x;
  if (tid < 5 * BP_RTAPS) kk[tid >> 4][tid & 15] = coeffs.k[tid >> 4][tid & 15];

  // 1. the HR patch: patch row r is image row 4 ty0 - 6 + r, patch byte q of it is byte 12 tx0 - 32 + q of that image row
  const int row_bytes = 12 * w;                                      // 3 * 4w
  const unsigned char* src = scratch + im.scr;                       // O: 256-byte aligned
  const bool rows_aligned = (w & 3) == 0;
  for (int i = tid; i < BP_PROWS * BP_PVEC; i += BP_THREADS) {
    const int r = i / BP_PVEC, v = i - r * BP_PVEC;
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
    *reinterpret_cast<uint4*>(patch + r * BP_PSTRIDE + 16 * v) = val;
  }
  __syncthreads();

  // 2. horizontal pass: column x of the tile, rows tid / 32 + 8 it.  The window of output tx0 + x begins at image byte
  //    12 (tx0 + x) - 18 = patch byte 12 x + 14: the 13 dwords from patch byte 12 x + 12 hold it from their byte 2 on.
  {
    const int x = tid & (BP_TW - 1);
    int kx[BP_RTAPS];
    const int4* kv = reinterpret_cast<const int4*>(kk[x4_down_vector(tx0 + x, w)]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 c = kv[q];
      kx[4 * q] = c.x, kx[4 * q + 1] = c.y, kx[4 * q + 2] = c.z, kx[4 * q + 3] = c.w;
    }
    for (int r = tid / BP_TW; r < BP_PROWS; r += BP_THREADS / BP_TW) {
      const unsigned* p = reinterpret_cast<const unsigned*>(patch + r * BP_PSTRIDE + 12 * x + 12);
      unsigned d[13];
#pragma unroll
      for (int q = 0; q < 13; ++q) d[q] = p[q];
      int acc[3] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
#pragma unroll
      for (int t = 0; t < BP_RTAPS; ++t) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += __mul24(kx[t], u8_of(d, 2 + 3 * t + c));
      }
      unsigned char* o = hbuf + r * BP_HSTRIDE + 3 * x;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (unsigned char)clip8(acc[c]);
    }
  }
  __syncthreads();

  // 3. vertical pass on the rounded bytes: an item is dword j of LR row yl of the tile = elements 4 j .. 4 j + 3 of that row
  unsigned char* down = scratch + im.scr + 2ull * bp_plane(h, w);
  for (int i = tid; i < BP_TH * BP_HDWORDS; i += BP_THREADS) {
    const int yl = i / BP_HDWORDS, j = i - yl * BP_HDWORDS;
    const int gy = ty0 + yl;
    if (gy >= h) continue;
    const int4* kv = reinterpret_cast<const int4*>(kk[x4_down_vector(gy, h)]);
    int ky[BP_RTAPS];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 c = kv[q];
      ky[4 * q] = c.x, ky[4 * q + 1] = c.y, ky[4 * q + 2] = c.z, ky[4 * q + 3] = c.w;
    }
    int acc[4] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
    const unsigned* p = reinterpret_cast<const unsigned*>(hbuf + 4 * yl * BP_HSTRIDE) + j;
#pragma unroll
    for (int t = 0; t < BP_RTAPS; ++t) {
      const unsigned d = p[t * BP_HDWORDS];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] += __mul24(ky[t], u8_of(&d, b));
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int e = 4 * j + b, px = e / 3, c = e - 3 * px;
      const int gx = tx0 + px;
      if (gx < w) down[((unsigned)gy * (unsigned)w + (unsigned)gx) * 3u + (unsigned)c] = (unsigned char)clip8(acc[b]);      // < 2^31 / 16
    }
  }
}

// O <- clip(O + C - U), U = x4 enlargement of D.
__global__ __launch_bounds__(BP_THREADS) void backproject_update_kernel(BpTable tab, BpUp coeffs, unsigned char* __restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) unsigned char dpatch[BP_DROWS * BP_DSTRIDE];
  __shared__ __attribute__((aligned(16))) unsigned char ubuf[BP_DROWS * BP_USTRIDE];
  __shared__ __attribute__((aligned(16))) int kk[16][BP_UTAPS];
  const BpImage im = tab.im[blockIdx.y];
  const int h = im.h, w = im.w;
  const unsigned tiles_x = bp_tiles_x(w);
  if (blockIdx.x >= tiles_x * bp_tiles_y(h)) return;
  const int tile_x = (int)(blockIdx.x % tiles_x);
  const int tx0 = tile_x * BP_TW, ty0 = (int)(blockIdx.x / tiles_x) * BP_TH;
  const int tid = (int)threadIdx.x;
  if (tid < 16 * BP_UTAPS) kk[tid >> 2][tid & 3] = coeffs.k[tid >> 2][tid & 3];

  // 1. the D patch: patch row r is LR row ty0 - 2 + r, patch pixel p of it is LR column tx0 - 2 + p; zeros outside the image
  const unsigned char* down = scratch + im.scr + 2ull * bp_plane(h, w);
  for (int i = tid; i < BP_DROWS * BP_DSTRIDE; i += BP_THREADS) {
    const int r = i / BP_DSTRIDE, b = i - r * BP_DSTRIDE;
    const int p = b / 3, c = b - 3 * p;
    const int y = ty0 - 2 + r, x = tx0 - 2 + p;
    unsigned char val = 0;
    if (b < BP_DBYTES && y >= 0 && y < h && x >= 0 && x < w) val = down[((unsigned)y * (unsigned)w + (unsigned)x) * 3u + (unsigned)c];
    dpatch[i] = val;
  }
  __syncthreads();

  // 2. horizontal pass: HR column x of the tile, rows tid / 128 + 2 it.  The frame of output 4 tx0 + x begins at LR column
  //    tx0 + floor((x - 6) / 4) = patch pixel (x + 2) >> 2: the 4 dwords from that pixel's dword hold its 12 bytes.
  {
    const int x = tid & (BP_UW - 1);
    const int4 kx4 = *reinterpret_cast<const int4*>(kk[x4_up_vector(4 * tx0 + x, 4 * w)]);
    const int kx[BP_UTAPS] = {kx4.x, kx4.y, kx4.z, kx4.w};
    const int first = 3 * ((x + 2) >> 2), skip = first & 3;
    for (int r = tid / BP_UW; r < BP_DROWS; r += BP_THREADS / BP_UW) {
      const unsigned* p = reinterpret_cast<const unsigned*>(dpatch + r * BP_DSTRIDE + (first & ~3));
      const unsigned d[4] = {p[0], p[1], p[2], p[3]};
      int acc[3] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
#pragma unroll
      for (int t = 0; t < BP_UTAPS; ++t) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += __mul24(kx[t], u8_of(d, skip + 3 * t + c));
      }
      unsigned char* o = ubuf + r * BP_USTRIDE + 3 * x;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (unsigned char)clip8(acc[c]);
    }
  }
  __syncthreads();

  // 3. vertical pass and the correction: an item is dword j of HR row y of the tile = bytes 384 tile_x + 4 j .. + 3 of image row
  //    4 ty0 + y.  The frame of that row begins at LR row ty0 + floor((y - 6) / 4) = patch row (y + 2) >> 2.
  const int row_bytes = 12 * w;
  unsigned char* o_u8 = scratch + im.scr;
  const unsigned char* c_u8 = o_u8 + bp_plane(h, w);
  for (int i = tid; i < BP_UH * BP_UDWORDS; i += BP_THREADS) {
    const int y = i / BP_UDWORDS, j = i - y * BP_UDWORDS;
    const int gy = 4 * ty0 + y, gb = BP_USTRIDE * tile_x + 4 * j;
    if (gy >= 4 * h || gb >= row_bytes) continue;                    // 12 w is a multiple of 4: a dword never straddles a row's end
    const int4 ky4 = *reinterpret_cast<const int4*>(kk[x4_up_vector(gy, 4 * h)]);
    const int ky[BP_UTAPS] = {ky4.x, ky4.y, ky4.z, ky4.w};
    int acc[4] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
    const unsigned* p = reinterpret_cast<const unsigned*>(ubuf + ((y + 2) >> 2) * BP_USTRIDE) + j;
#pragma unroll
    for (int t = 0; t < BP_UTAPS; ++t) {
      const unsigned d = p[t * BP_UDWORDS];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] += __mul24(ky[t], u8_of(&d, b));
    }
    const size_t g = (size_t)gy * (size_t)row_bytes + (size_t)gb;    // < 48 h w
    const unsigned ov = *reinterpret_cast<const unsigned*>(o_u8 + g), cv = *reinterpret_cast<const unsigned*>(c_u8 + g);
    unsigned res = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int v = u8_of(&ov, b) + u8_of(&cv, b) - clip8(acc[b]);
      res |= (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * b);
    }
    *reinterpret_cast<unsigned*>(o_u8 + g) = res;
  }
}

int backproject_images(const char* who, const float* out01, const float* cond01, const int64_t* offsets, const int32_t* hw, int n_images,
                       int iterations, float* dst01, void* scratch, hipStream_t st) {
  const std::string name(who);
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!out01 || !cond01 || !offsets || !hw || !dst01 || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (iterations < 1 || iterations > BP_MAX_ITERATIONS) SRGD_EXT_FAIL(name + ": iterations outside 1 .. 64");
  if ((((uintptr_t)out01 | (uintptr_t)cond01 | (uintptr_t)dst01) & 3u) != 0) SRGD_EXT_FAIL(name + ": out01, cond01 and dst01 must be 4-byte aligned");
  if (((uintptr_t)scratch & 255u) != 0) SRGD_EXT_FAIL(name + ": scratch must be 256-byte aligned");
  long long lo = 0, hi = 0;                              // the elements the call covers in each of the three buffers: [lo, hi)
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const long long h = hw[2 * i], w = hw[2 * i + 1];
    if (h < 5 || w < 5) SRGD_EXT_FAIL(name + ": bad size (h and w must be >= 5: smaller windows overlap and depend on the size)");
    if (48 * h * w >= 0x7fffff00ll) SRGD_EXT_FAIL(name + ": output of 2^31 - 256 elements or more");
    if (offsets[i] < 0 || offsets[i] >= (1ll << 40)) SRGD_EXT_FAIL(name + ": offset outside [0, 2^40)");
    lo = i == 0 ? offsets[i] : std::min<long long>(lo, offsets[i]);
    hi = i == 0 ? offsets[i] + 48 * h * w : std::max<long long>(hi, offsets[i] + 48 * h * w);
  }
  const long long span = 4 * (hi - lo);                  // bytes
  const long long to_out = (long long)((intptr_t)dst01 - (intptr_t)out01), to_cond = (long long)((intptr_t)dst01 - (intptr_t)cond01);
  if (to_out != 0 && to_out < span && -to_out < span) SRGD_EXT_FAIL(name + ": partial overlap of dst01 and out01 (dst01 == out01 is in place)");
  if (to_cond < span && -to_cond < span) SRGD_EXT_FAIL(name + ": overlap of dst01 and cond01");
  static const BpDown down = [] {                        // pillow_coeffs.hpp: the vectors on the frames of their outputs
    BpDown c;
    pillow::x4_reduce_vectors(c.k, true);
    return c;
  }();
  static const BpUp up = [] {
    BpUp c;
    pillow::x4_enlarge_vectors(c.k, true);
    return c;
  }();
  unsigned long long scr = 0;                            // the images' scratch, packed in image order
  for (int first = 0; first < n_images; first += BP_MAX_IMAGES) {     // one launch sequence per BP_MAX_IMAGES images
    const int cnt = std::min(BP_MAX_IMAGES, n_images - first);
    BpTable tab;
    unsigned max_tiles = 0, max_quads = 0;
    for (int k = 0; k < BP_MAX_IMAGES; ++k) tab.im[k] = BpImage{0ll, 0ull, 0, 0};
    for (int k = 0; k < cnt; ++k) {
      const int i = first + k;
      const int h = hw[2 * i], w = hw[2 * i + 1];
      tab.im[k] = BpImage{(long long)offsets[i], scr, h, w};
      scr += bp_scratch(h, w);
      max_tiles = std::max(max_tiles, bp_tiles_x(w) * bp_tiles_y(h));
      max_quads = std::max(max_quads, 4u * (unsigned)h * (unsigned)w);
    }
    const dim3 flat(std::min((max_quads + BP_THREADS - 1) / BP_THREADS, 8192u), (unsigned)cnt), tiles(max_tiles, (unsigned)cnt);
    hipLaunchKernelGGL(backproject_begin_kernel, flat, dim3(BP_THREADS), 0, st, tab, out01, cond01, (unsigned char*)scratch);
    for (int it = 0; it < iterations; ++it) {
      hipLaunchKernelGGL(backproject_reduce_kernel, tiles, dim3(BP_THREADS), 0, st, tab, down, (unsigned char*)scratch);
      hipLaunchKernelGGL(backproject_update_kernel, tiles, dim3(BP_THREADS), 0, st, tab, up, (unsigned char*)scratch);
    }
    hipLaunchKernelGGL(backproject_end_kernel, flat, dim3(BP_THREADS), 0, st, tab, out01, dst01, (const unsigned char*)scratch);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_image_backproject_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_image_backproject_coeffs(int32_t out[16][4]) {
  if (!out) SRGD_EXT_FAIL("srgd_image_backproject_coeffs: null argument");
  pillow::x4_enlarge_vectors(out, false);
  return 0;
}

SRGD_EXT_EXPORT int srgd_image_backproject(const float* out01, const float* cond01, int h, int w, int iterations, float* dst01, void* scratch,
                                           void* stream) {
  const int64_t off = 0;
  const int32_t hw[2] = {h, w};
  return backproject_images("srgd_image_backproject", out01, cond01, &off, hw, 1, iterations, dst01, scratch, (hipStream_t)stream);
}

SRGD_EXT_EXPORT int srgd_image_backproject_images(const float* out01, const float* cond01, const int64_t* offsets_host, const int32_t* hw_host,
                                                  int n_images, int iterations, float* dst01, void* scratch, void* stream) {
  return backproject_images("srgd_image_backproject_images", out01, cond01, offsets_host, hw_host, n_images, iterations, dst01, scratch,
                            (hipStream_t)stream);
}

}  // extern "C"
