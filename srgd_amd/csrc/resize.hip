// Pillow-exact resize of 8-bit RGB images by any ratio up to 8 either way on the GPU (engine extension, absent upstream): what
// PIL.Image.resize((w_out, h_out), BICUBIC | BILINEAR | LANCZOS) gives, bit for bit.  The definition is fixed in
// include/srgd_resize.h and restated here in short: per axis a table of clipped, renormalised windows in 22-bit fixed point
// (computed on the host in double, in Pillow's order), the horizontal pass over all input rows rounded to 8 bits, then the vertical
// pass on that result; a pass whose in == out is skipped.
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument), blockIdx.x the tile.
//   horizontal: one workgroup of 256 threads per tile of 32 output pixels x 16 rows.  The tile's bounds and coefficient rows (at most
//               32 x 49 ints) and the bytes of its rows between the first window's first pixel and the last window's end (at most
//               3 * (31 * 8 + 2 * 24 + 1) = 891 bytes, from the dword in front of them) go to LDS; a thread owns one output pixel
//               of rows r and r + 8: its coefficient is read once per tap and serves six products; results go to LDS as bytes and
//               leave as whole dwords along the row.
//   vertical:   one workgroup per tile of 256 bytes x 16 output rows.  The bounds and coefficient rows of the 16 outputs go to LDS; a
//               thread owns dword j of the tile's rows r, r + 4, ...: every tap is one dword load along the contiguous byte axis and
//               four products with one coefficient, the result one dword store.  With no table at all (both passes skipped) the same
//               kernel copies: one tap of 2^22 at the output's own row.
// Rows are 3 w bytes: with w % 4 != 0 they are not dword aligned and the image takes the guarded byte path of each kernel.
// Every index a kernel reads from a table is clamped to the image and to the staged span before use, and every store is guarded by
// the sizes of the (host-checked) record: no table content can make a kernel read or write outside its image.
// No atomics, no reductions: every byte depends on its own image alone - bit-identical alone, in any group, at any offset.
// LDS: horizontal 14,656 (rows) + 6,272 (coefficients) + 256 (bounds) + 1,536 (result) = 22,720 bytes; vertical 3,136 + 128.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_resize.h"
#include "ext_common.hpp"

// This file is a library of its own (libsrgd_resize.so, include/srgd_resize.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing.
namespace srgd {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_IMAGES = 128;                   // records travel as a kernel argument (3.5 KiB)
constexpr int RS_MAX_TAPS = SRGD_RESIZE_MAX_TAPS;
constexpr int RS_HW = 32, RS_HR = 16;                // horizontal tile: output pixels x rows
constexpr int RS_HSPAN = 916;                        // LDS bytes of a staged source row: 229 dwords (odd: rows fall on different banks)
constexpr int RS_HOUT = 3 * RS_HW;                   // bytes of a tile row of the result: 96
constexpr int RS_VB = 256, RS_VR = 16;               // vertical tile: bytes x output rows
static_assert(3 * ((RS_HW - 1) * SRGD_RESIZE_MAX_RATIO + 2 * 3 * SRGD_RESIZE_MAX_RATIO + 1) + 3 + 3 <= RS_HSPAN,
              "the widest span of a tile, from the dword in front of it to the dword behind it, fits a staged row");
static_assert(RS_THREADS == RS_HW * (RS_HR / 2), "horizontal pass: a thread per output pixel and pair of rows");
static_assert(RS_THREADS == (RS_VB / 4) * 4 && RS_VR % 4 == 0, "vertical pass: a thread per dword, four rows at a time");
static_assert(2 * (int)(3 * SRGD_RESIZE_MAX_RATIO) + 1 == RS_MAX_TAPS, "lanczos at 8 : 1 is the widest table");
static_assert(SRGD_RESIZE_LANCZOS == pillow::LANCZOS && SRGD_RESIZE_BILINEAR == pillow::BILINEAR && SRGD_RESIZE_BICUBIC == pillow::BICUBIC &&
              RS_MAX_TAPS <= pillow::MAX_TAPS, "the filters and the widest table of pillow_coeffs.hpp");

struct RsImage {                                     // offsets in units of 16 bytes: [0, 2^36) bytes
  unsigned src16, dst16, scr16, tab16;
  unsigned short h_in, w_in, h_out, w_out;           // 1 .. 16384
  unsigned char kh, kv, pad0, pad1;                  // ksize of the two tables; 0: the pass is skipped
};
struct RsTable { RsImage im[RS_MAX_IMAGES]; };
static_assert(sizeof(RsTable) <= 3584, "the records and five pointers stay below 4 KiB of kernel arguments");

// Horizontal pass: src -> scratch (-> dst where the vertical pass is skipped).
__global__ __launch_bounds__(RS_THREADS) void resize_horizontal_kernel(RsTable tab, const unsigned char* __restrict__ src,
                                                                       unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                       const unsigned char* __restrict__ tables) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[RS_HR * RS_HSPAN];
  __shared__ __attribute__((aligned(16))) int kk[RS_HW * RS_MAX_TAPS];
  __shared__ __attribute__((aligned(16))) int bnd[2 * RS_HW];
  __shared__ __attribute__((aligned(16))) unsigned char res[RS_HR * RS_HOUT];
  const RsImage im = tab.im[blockIdx.y];
  const int kh = im.kh, h_in = im.h_in, w_in = im.w_in, w_out = im.w_out;
  if (kh == 0) return;                                               // no horizontal pass for this image
  const unsigned tiles_x = (unsigned)(w_out + RS_HW - 1) / RS_HW, tiles_y = (unsigned)(h_in + RS_HR - 1) / RS_HR;
  if (blockIdx.x >= tiles_x * tiles_y) return;                       // the grid is as wide as the launch's largest image
  const int x0 = (int)(blockIdx.x % tiles_x) * RS_HW, y0 = (int)(blockIdx.x / tiles_x) * RS_HR;
  const int nx = min(RS_HW, w_out - x0), ny = min(RS_HR, h_in - y0);
  const int tid = (int)threadIdx.x;

  // 1. the tile's bounds and coefficient rows (the rows keep their stride kh, an odd number of dwords)
  const int* tb = reinterpret_cast<const int*>(tables + 16ull * im.tab16);
  const int* tc = tb + 2 * w_out;
  for (int i = tid; i < 2 * nx; i += RS_THREADS) bnd[i] = tb[2 * x0 + i];
  for (int i = tid; i < nx * kh; i += RS_THREADS) kk[i] = tc[x0 * kh + i];
  __syncthreads();

  // 2. the source span of the tile's rows: bytes [a0, b1) of image rows y0 .. y0 + ny - 1, a0 a multiple of 4 on the dword path
  const unsigned char* in = src + 16ull * im.src16;
  const int in_bytes = 3 * w_in;
  const bool in_dwords = (w_in & 3) == 0 && ((uintptr_t)in & 3u) == 0;
  const int first = min(max(bnd[0], 0), w_in - 1);
  const int last_end = min(max(bnd[2 * (nx - 1)] + bnd[2 * (nx - 1) + 1], first), w_in);
  const int a0 = in_dwords ? ((3 * first) & ~3) : 3 * first;
  const int span = min(3 * last_end - a0, RS_HSPAN);                 // staged bytes of a row (<= 891 + 3 for every table of the library)
  if (in_dwords) {
    const int nd = (span + 3) >> 2;                                  // a0 + 4 nd <= in_bytes: both are multiples of 4 and a0 + span <= in_bytes
    for (int i = tid; i < ny * nd; i += RS_THREADS) {
      const int r = i / nd, d = i - r * nd;
      *reinterpret_cast<unsigned*>(rows + r * RS_HSPAN + 4 * d) =
          *reinterpret_cast<const unsigned*>(in + (size_t)(y0 + r) * (size_t)in_bytes + (size_t)(a0 + 4 * d));
    }
  } else {
    for (int i = tid; i < ny * span; i += RS_THREADS) {
      const int r = i / span, b = i - r * span;
      rows[r * RS_HSPAN + b] = in[(size_t)(y0 + r) * (size_t)in_bytes + (size_t)(a0 + b)];
    }
  }
  __syncthreads();

  // 3. output pixel x of the tile, rows rg and rg + 8
  {
    const int x = tid & (RS_HW - 1), rg = tid / RS_HW;
    if (x < nx) {
      const int xmin = min(max(bnd[2 * x], first), w_in - 1);
      const int off = 3 * xmin - a0;                                 // >= 0
      const int count = max(min(min(bnd[2 * x + 1], kh), (span - off) / 3), 0);      // every tap lies inside the staged span
      const unsigned char* p0 = rows + rg * RS_HSPAN + off;
      const unsigned char* p1 = p0 + (RS_HR / 2) * RS_HSPAN;
      const int* k = kk + x * kh;
      int acc0[3] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
      int acc1[3] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
      for (int t = 0; t < count; ++t) {
        const int kt = k[t];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          acc0[c] += kt * (int)p0[3 * t + c];
          acc1[c] += kt * (int)p1[3 * t + c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        res[rg * RS_HOUT + 3 * x + c] = (unsigned char)clip8(acc0[c]);
        res[(rg + RS_HR / 2) * RS_HOUT + 3 * x + c] = (unsigned char)clip8(acc1[c]);
      }
    }
  }
  __syncthreads();

  // 4. the tile's result: bytes [3 x0, 3 x0 + 3 nx) of rows y0 .. y0 + ny - 1 of [h_in][w_out][3]
  unsigned char* out = im.kv == 0 ? dst + 16ull * im.dst16 : scratch + 16ull * im.scr16;
  const int out_bytes = 3 * w_out, nb = 3 * nx;
  if ((w_out & 3) == 0 && ((uintptr_t)out & 3u) == 0) {              // 3 x0 = 96 tile and 3 nx are multiples of 4
    const int nd = nb >> 2;
    for (int i = tid; i < ny * nd; i += RS_THREADS) {
      const int r = i / nd, d = i - r * nd;
      *reinterpret_cast<unsigned*>(out + (size_t)(y0 + r) * (size_t)out_bytes + (size_t)(3 * x0 + 4 * d)) =
          *reinterpret_cast<const unsigned*>(res + r * RS_HOUT + 4 * d);
    }
  } else {
    for (int i = tid; i < ny * nb; i += RS_THREADS) {
      const int r = i / nb, b = i - r * nb;
      out[(size_t)(y0 + r) * (size_t)out_bytes + (size_t)(3 * x0 + b)] = res[r * RS_HOUT + b];
    }
  }
}

// Vertical pass: scratch (src where the horizontal pass is skipped) -> dst; the copy where both are skipped.
__global__ __launch_bounds__(RS_THREADS) void resize_vertical_kernel(RsTable tab, const unsigned char* __restrict__ src,
                                                                     const unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                     const unsigned char* __restrict__ tables) {
  __shared__ __attribute__((aligned(16))) int kk[RS_VR * RS_MAX_TAPS];
  __shared__ __attribute__((aligned(16))) int bnd[2 * RS_VR];
  const RsImage im = tab.im[blockIdx.y];
  const int kh = im.kh, kv = im.kv, h_in = im.h_in, h_out = im.h_out, w_out = im.w_out;
  if (kv == 0 && kh != 0) return;                                    // the horizontal pass wrote the destination
  const int row_bytes = 3 * w_out;
  const unsigned tiles_x = (unsigned)(row_bytes + RS_VB - 1) / RS_VB, tiles_y = (unsigned)(h_out + RS_VR - 1) / RS_VR;
  if (blockIdx.x >= tiles_x * tiles_y) return;
  const int gb = (int)(blockIdx.x % tiles_x) * RS_VB + 4 * ((int)threadIdx.x & (RS_VB / 4 - 1));
  const int y0 = (int)(blockIdx.x / tiles_x) * RS_VR;
  const int ny = min(RS_VR, h_out - y0);
  const int tid = (int)threadIdx.x;
  if (kv != 0) {                                                     // the table h_in -> h_out follows the table w_in -> w_out
    const int* tb = reinterpret_cast<const int*>(tables + 16ull * im.tab16) + (kh != 0 ? w_out * (2 + kh) : 0);
    const int* tc = tb + 2 * h_out;
    for (int i = tid; i < 2 * ny; i += RS_THREADS) bnd[i] = tb[2 * y0 + i];
    for (int i = tid; i < ny * kv; i += RS_THREADS) kk[i] = tc[y0 * kv + i];
  }
  __syncthreads();
  if (gb >= row_bytes) return;
  const unsigned char* in = kh != 0 ? scratch + 16ull * im.scr16 : src + 16ull * im.src16;
  unsigned char* out = dst + 16ull * im.dst16;
  const bool dwords = (w_out & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 3u) == 0;       // gb + 4 <= row_bytes then
  const int nbytes = min(4, row_bytes - gb);
  for (int r = tid / (RS_VB / 4); r < ny; r += RS_THREADS / (RS_VB / 4)) {
    const int yo = y0 + r;
    const int ymin = kv != 0 ? min(max(bnd[2 * r], 0), h_in - 1) : yo;
    const int count = kv != 0 ? max(min(min(bnd[2 * r + 1], kv), h_in - ymin), 0) : 1;
    const int* k = kk + r * kv;
    int acc[4] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
    const unsigned char* p = in + (size_t)ymin * (size_t)row_bytes + (size_t)gb;
    for (int t = 0; t < count; ++t, p += row_bytes) {
      const int kt = kv != 0 ? k[t] : 1 << PILLOW_PREC_BITS;
      unsigned d = 0u;
      if (dwords) {
        d = *reinterpret_cast<const unsigned*>(p);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (b < nbytes) d |= (unsigned)p[b] << (8 * b);
        }
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] += kt * (int)((d >> (8 * b)) & 0xffu);
    }
    unsigned char* o = out + (size_t)yo * (size_t)row_bytes + (size_t)gb;
    if (dwords) {
      *reinterpret_cast<unsigned*>(o) = (unsigned)clip8(acc[0]) | (unsigned)clip8(acc[1]) << 8 | (unsigned)clip8(acc[2]) << 16 |
                                        (unsigned)clip8(acc[3]) << 24;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b < nbytes) o[b] = (unsigned char)clip8(acc[b]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host (Pillow's tables: pillow_coeffs.hpp)
const char* axis_problem(long long in_size, long long out_size) {
  if (in_size < 1 || out_size < 1 || in_size > SRGD_RESIZE_MAX_SIDE || out_size > SRGD_RESIZE_MAX_SIDE) return "bad size (every size is in 1 .. 16384)";
  if (in_size > SRGD_RESIZE_MAX_RATIO * out_size || out_size > SRGD_RESIZE_MAX_RATIO * in_size) return "ratio out of range (at most 8 either way, per axis)";
  return nullptr;
}

int resize_images(const void* src, void* dst, const srgd_resize_image* images, int n_images, int filter, const void* tables,
                  long long tables_bytes, void* scratch, long long scratch_bytes, hipStream_t st) {
  const std::string name("srgd_resize_u8_images");
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!src || !dst || !images || !tables || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (pillow::filter_support(filter) == 0.0) SRGD_EXT_FAIL(name + ": unknown filter (1 lanczos, 2 bilinear, 3 bicubic)");
  if (((uintptr_t)scratch & 15u) != 0) SRGD_EXT_FAIL(name + ": scratch must be 16-byte aligned");
  if (((uintptr_t)tables & 15u) != 0) SRGD_EXT_FAIL(name + ": tables must be 16-byte aligned");
  long long scr = 0, src_lo = 0, src_hi = 0, dst_lo = 0, dst_hi = 0;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const srgd_resize_image& im = images[i];
    const char* problem = axis_problem(im.h_in, im.h_out);
    if (!problem) problem = axis_problem(im.w_in, im.w_out);
    if (problem) SRGD_EXT_FAIL(name + ": " + problem);
    for (const long long off : {(long long)im.src_off, (long long)im.dst_off, (long long)im.tab_off}) {
      if (off < 0 || off >= (1ll << 36)) SRGD_EXT_FAIL(name + ": offset outside [0, 2^36)");
      if ((off & 15) != 0) SRGD_EXT_FAIL(name + ": offset is not a multiple of 16");
    }
    long long need = 0;                                  // bytes of the image's tables
    if (im.w_in != im.w_out) need += 4ll * im.w_out * (2 + pillow::ksize(im.w_in, im.w_out, filter));
    if (im.h_in != im.h_out) need += 4ll * im.h_out * (2 + pillow::ksize(im.h_in, im.h_out, filter));
    if (im.tab_off + need > tables_bytes) SRGD_EXT_FAIL(name + ": tables_bytes is too small for the images' tables");
    scr += round_up(3ll * im.h_in * im.w_out, 16ll);
    const long long s_end = im.src_off + 3ll * im.h_in * im.w_in, d_end = im.dst_off + 3ll * im.h_out * im.w_out;
    src_lo = i == 0 ? (long long)im.src_off : std::min<long long>(src_lo, im.src_off);
    src_hi = i == 0 ? s_end : std::max(src_hi, s_end);
    dst_lo = i == 0 ? (long long)im.dst_off : std::min<long long>(dst_lo, im.dst_off);
    dst_hi = i == 0 ? d_end : std::max(dst_hi, d_end);
  }
  if (scr > scratch_bytes) SRGD_EXT_FAIL(name + ": scratch_bytes is too small (sum of 3 * h_in * w_out, each rounded up to 16)");
  if (scr > (1ll << 36)) SRGD_EXT_FAIL(name + ": scratch beyond 2^36 bytes");
  const long long s0 = (long long)(intptr_t)src + src_lo, s1 = (long long)(intptr_t)src + src_hi;
  const long long d0 = (long long)(intptr_t)dst + dst_lo, d1 = (long long)(intptr_t)dst + dst_hi;
  if (s0 < d1 && d0 < s1) SRGD_EXT_FAIL(name + ": the source images and the destination images overlap");
  scr = 0;                                               // the images' scratch, packed in image order
  for (int first = 0; first < n_images; first += RS_MAX_IMAGES) {     // one launch sequence per RS_MAX_IMAGES images
    const int cnt = std::min(RS_MAX_IMAGES, n_images - first);
    RsTable tab;
    unsigned h_tiles = 0, v_tiles = 0;
    for (int k = 0; k < RS_MAX_IMAGES; ++k) tab.im[k] = RsImage{0u, 0u, 0u, 0u, 1, 1, 1, 1, 0, 0, 0, 0};
    for (int k = 0; k < cnt; ++k) {
      const srgd_resize_image& im = images[first + k];
      const int kh = im.w_in != im.w_out ? pillow::ksize(im.w_in, im.w_out, filter) : 0;
      const int kv = im.h_in != im.h_out ? pillow::ksize(im.h_in, im.h_out, filter) : 0;
      tab.im[k] = RsImage{(unsigned)(im.src_off >> 4), (unsigned)(im.dst_off >> 4), (unsigned)(scr >> 4), (unsigned)(im.tab_off >> 4),
                          (unsigned short)im.h_in, (unsigned short)im.w_in, (unsigned short)im.h_out, (unsigned short)im.w_out,
                          (unsigned char)kh, (unsigned char)kv, 0, 0};
      scr += round_up(3ll * im.h_in * im.w_out, 16ll);
      if (kh != 0) h_tiles = std::max(h_tiles, (unsigned)((im.w_out + RS_HW - 1) / RS_HW) * (unsigned)((im.h_in + RS_HR - 1) / RS_HR));
      if (kv != 0 || kh == 0)
        v_tiles = std::max(v_tiles, (unsigned)((3 * im.w_out + RS_VB - 1) / RS_VB) * (unsigned)((im.h_out + RS_VR - 1) / RS_VR));
    }
    if (h_tiles != 0)
      hipLaunchKernelGGL(resize_horizontal_kernel, dim3(h_tiles, (unsigned)cnt), dim3(RS_THREADS), 0, st, tab, (const unsigned char*)src,
                         (unsigned char*)scratch, (unsigned char*)dst, (const unsigned char*)tables);
    if (v_tiles != 0)
      hipLaunchKernelGGL(resize_vertical_kernel, dim3(v_tiles, (unsigned)cnt), dim3(RS_THREADS), 0, st, tab, (const unsigned char*)src,
                         (const unsigned char*)scratch, (unsigned char*)dst, (const unsigned char*)tables);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
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
