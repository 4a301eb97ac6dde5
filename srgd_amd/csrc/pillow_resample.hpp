// The general two-pass Pillow-exact 8-bit resize, once: the device bodies and the host driver behind resize.hip (3 channels) and
// alpha.hip (planes).  A header, not a library: each of the two includes it into its one translation unit, keeps its __global__ entry
// points under its own names, one per instantiated body (a body's LDS arrays are its kernel's), so the two libraries still share no symbol.
//
// The definition (include/srgd_resize.h): per axis a table of clipped, renormalised windows in 22-bit fixed point, the horizontal pass
// over all input rows rounded to 8 bits, then the vertical pass on that result; a pass whose in == out is skipped.
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument), blockIdx.x the tile.
//   horizontal: one workgroup of 256 threads per tile of HW output pixels x 16 rows of C channels.  The tile's bounds and coefficient
//               rows (at most HW x 49 ints) and the bytes of its rows between the first window's first pixel and the last window's
//               end (at most C * ((HW - 1) * 8 + 2 * 24 + 1) bytes, from the dword in front of them) go to LDS; a thread owns one
//               output pixel of R rows, 16 / R apart: its coefficient is read once per tap and serves R * C products; results go to
//               LDS as bytes and leave as whole dwords along the row.
//   vertical:   one workgroup per tile of 256 bytes x 16 output rows.  The bounds and coefficient rows of the 16 outputs go to LDS; a
//               thread owns dword j of the tile's rows r, r + 4, ...: every tap is one dword load along the contiguous byte axis and
//               four products with one coefficient, the result one dword store.  With no table at all (both passes skipped) the same
//               kernel copies: one tap of 2^22 at the output's own row.
// Rows are C w bytes: with w % 4 != 0 they are not dword aligned and the image takes the guarded byte path of each kernel; so does an
// image whose base is not, unless ALIGNED says that the host has checked the bases to 16 bytes.
// Every index a kernel reads from a table is clamped to the image and to the staged span before use, and every store is guarded by
// the sizes of the (host-checked) record: no table content can make a kernel read or write outside its image.
// No atomics, no reductions: every byte depends on its own image alone - bit-identical alone, in any group, at any offset.
#pragma once

#include <algorithm>
#include <string>

#include <hip/hip_runtime.h>

#include "ext_common.hpp"

namespace srgd {
namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_IMAGES = 128;                   // records travel as a kernel argument (3.5 KiB)
constexpr int PR_MAX_SIDE = 16384, PR_MAX_RATIO = 8;
constexpr int PR_MAX_TAPS = 49;
constexpr int PR_HALF = 1 << (PILLOW_PREC_BITS - 1);                // an accumulator begins at one half: Pillow's rounding
constexpr int PR_HR = 16;                            // rows of a horizontal tile
constexpr int PR_VB = 256, PR_VR = 16;               // vertical tile: bytes x output rows
static_assert(PR_THREADS == (PR_VB / 4) * 4 && PR_VR % 4 == 0, "vertical pass: a thread per dword, four rows at a time");
static_assert(2 * (int)(3 * PR_MAX_RATIO) + 1 == PR_MAX_TAPS && PR_MAX_TAPS <= pillow::MAX_TAPS, "lanczos at 8 : 1 is the widest table");

struct PrImage {                                     // offsets in units of 16 bytes: [0, 2^36) bytes
  unsigned src16, dst16, scr16, tab16;
  unsigned short h_in, w_in, h_out, w_out;           // 1 .. 16384
  unsigned char kh, kv, pad0, pad1;                  // ksize of the two tables; 0: the pass is skipped
};
struct PrTable { PrImage im[PR_MAX_IMAGES]; };
static_assert(sizeof(PrTable) <= 3584, "the records and five pointers stay below 4 KiB of kernel arguments");

// The horizontal tile of C channels, HW output pixels and R rows per thread: the sizes of its four LDS arrays.
template <int C, int HW, int R>
struct PrHTile {
  static constexpr int WIDEST = C * ((HW - 1) * PR_MAX_RATIO + 2 * 3 * PR_MAX_RATIO + 1) + 3 + 3;
  static constexpr int SPAN = round_up(WIDEST, 16) + 4;              // LDS bytes of a staged source row: an odd number of dwords (rows fall on different banks)
  static constexpr int OUT = C * HW;                                 // bytes of a tile row of the result
  static constexpr int ROWS = PR_HR * SPAN, KK = HW * PR_MAX_TAPS, BND = 2 * HW, RES = PR_HR * OUT;
  static_assert(WIDEST <= SPAN && SPAN % 4 == 0,
                "the widest span of a tile, from the dword in front of it to the dword behind it, fits a staged row");
  static_assert((HW & (HW - 1)) == 0 && PR_HR % R == 0 && PR_THREADS == HW * (PR_HR / R), "horizontal pass: a thread per output pixel and R rows");
  static_assert(OUT % 4 == 0, "a tile row of the result is whole dwords");
};

// Horizontal pass: src -> scratch (-> dst where the vertical pass is skipped).  The body of ONE kernel per instantiation: its LDS
// arrays are that kernel's.
template <int C, int HW, int R, bool ALIGNED>
__device__ __forceinline__ void pr_horizontal(const PrTable& tab, const unsigned char* __restrict__ src, unsigned char* __restrict__ scratch,
                                              unsigned char* __restrict__ dst, const unsigned char* __restrict__ tables) {
  using T = PrHTile<C, HW, R>;
  __shared__ __attribute__((aligned(16))) unsigned char rows[T::ROWS];
  __shared__ __attribute__((aligned(16))) int kk[T::KK];
  __shared__ __attribute__((aligned(16))) int bnd[T::BND];
  __shared__ __attribute__((aligned(16))) unsigned char res[T::RES];
  const PrImage im = tab.im[blockIdx.y];
  const int kh = im.kh, h_in = im.h_in, w_in = im.w_in, w_out = im.w_out;
  if (kh == 0) return;                                               // no horizontal pass for this image
  const unsigned tiles_x = (unsigned)(w_out + HW - 1) / HW, tiles_y = (unsigned)(h_in + PR_HR - 1) / PR_HR;
  if (blockIdx.x >= tiles_x * tiles_y) return;                       // the grid is as wide as the launch's largest image
  const int x0 = (int)(blockIdx.x % tiles_x) * HW, y0 = (int)(blockIdx.x / tiles_x) * PR_HR;
  const int nx = min(HW, w_out - x0), ny = min(PR_HR, h_in - y0);
  const int tid = (int)threadIdx.x;

  // 1. the tile's bounds and coefficient rows (the rows keep their stride kh, an odd number of dwords)
  const int* tb = reinterpret_cast<const int*>(tables + 16ull * im.tab16);
  const int* tc = tb + 2 * w_out;
  for (int i = tid; i < 2 * nx; i += PR_THREADS) bnd[i] = tb[2 * x0 + i];
  for (int i = tid; i < nx * kh; i += PR_THREADS) kk[i] = tc[x0 * kh + i];
  __syncthreads();

  // 2. the source span of the tile's rows: bytes [a0, a0 + span) of image rows y0 .. y0 + ny - 1, a0 a multiple of 4 on the dword path
  const unsigned char* in = src + 16ull * im.src16;
  const int in_bytes = C * w_in;
  const bool in_dwords = (w_in & 3) == 0 && (ALIGNED || ((uintptr_t)in & 3u) == 0);
  const int first = min(max(bnd[0], 0), w_in - 1);
  const int last_end = min(max(bnd[2 * (nx - 1)] + bnd[2 * (nx - 1) + 1], first), w_in);
  const int a0 = in_dwords ? ((C * first) & ~3) : C * first;
  const int span = min(C * last_end - a0, T::SPAN);                  // staged bytes of a row (<= WIDEST - 3 for every table within the ratio)
  if (in_dwords) {
    const int nd = (span + 3) >> 2;                                  // a0 + 4 nd <= in_bytes: both are multiples of 4 and a0 + span <= in_bytes
    for (int i = tid; i < ny * nd; i += PR_THREADS) {
      const int r = i / nd, d = i - r * nd;
      *reinterpret_cast<unsigned*>(rows + r * T::SPAN + 4 * d) =
          *reinterpret_cast<const unsigned*>(in + (size_t)(y0 + r) * (size_t)in_bytes + (size_t)(a0 + 4 * d));
    }
  } else {
    for (int i = tid; i < ny * span; i += PR_THREADS) {
      const int r = i / span, b = i - r * span;
      rows[r * T::SPAN + b] = in[(size_t)(y0 + r) * (size_t)in_bytes + (size_t)(a0 + b)];
    }
  }
  __syncthreads();

  // 3. output pixel x of the tile, rows rg + q * 16 / R (rows beyond ny hold stale LDS bytes and are never stored)
  {
    const int x = tid & (HW - 1), rg = tid / HW;
    if (x < nx) {
      const int xmin = min(max(bnd[2 * x], first), w_in - 1);
      const int off = C * xmin - a0;                                 // >= 0
      const int count = max(min(min(bnd[2 * x + 1], kh), (span - off) / C), 0);      // every tap lies inside the staged span
      // tap 0 of the thread's R rows, as one pointer and constants from it: the loads of a tap then share an address register, and
      // the tap loop keeps its short form (R pointers computed apart cost resize 2 VGPRs, an index q * stride + t 12, and alpha 20)
      const unsigned char* p[R];
      p[0] = rows + rg * T::SPAN + off;
#pragma unroll
      for (int q = 1; q < R; ++q) p[q] = p[0] + q * (PR_HR / R) * T::SPAN;
      const int* k = kk + x * kh;
      int acc[R][C];
#pragma unroll
      for (int q = 0; q < R; ++q) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[q][c] = PR_HALF;
      }
      for (int t = 0; t < count; ++t) {
        const int kt = k[t];
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
          for (int q = 0; q < R; ++q) acc[q][c] += kt * (int)p[q][C * t + c];
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int q = 0; q < R; ++q) res[(rg + q * (PR_HR / R)) * T::OUT + C * x + c] = (unsigned char)clip8(acc[q][c]);
      }
    }
  }
  __syncthreads();

  // 4. the tile's result: bytes [C x0, C x0 + C nx) of rows y0 .. y0 + ny - 1 of [h_in][w_out][C]
  unsigned char* out = im.kv == 0 ? dst + 16ull * im.dst16 : scratch + 16ull * im.scr16;
  const int out_bytes = C * w_out, nb = C * nx;
  if ((w_out & 3) == 0 && (ALIGNED || ((uintptr_t)out & 3u) == 0)) { // C x0, a multiple of the tile's OUT, and C nx are multiples of 4 then
    const int nd = nb >> 2;
    for (int i = tid; i < ny * nd; i += PR_THREADS) {
      const int r = i / nd, d = i - r * nd;
      *reinterpret_cast<unsigned*>(out + (size_t)(y0 + r) * (size_t)out_bytes + (size_t)(C * x0 + 4 * d)) =
          *reinterpret_cast<const unsigned*>(res + r * T::OUT + 4 * d);
    }
  } else {
    for (int i = tid; i < ny * nb; i += PR_THREADS) {
      const int r = i / nb, b = i - r * nb;
      out[(size_t)(y0 + r) * (size_t)out_bytes + (size_t)(C * x0 + b)] = res[r * T::OUT + b];
    }
  }
}

// Vertical pass: scratch (src where the horizontal pass is skipped) -> dst; the copy where both are skipped.  The body of ONE kernel
// per instantiation, as above.
template <int C, bool ALIGNED>
__device__ __forceinline__ void pr_vertical(const PrTable& tab, const unsigned char* __restrict__ src, const unsigned char* __restrict__ scratch,
                                            unsigned char* __restrict__ dst, const unsigned char* __restrict__ tables) {
  __shared__ __attribute__((aligned(16))) int kk[PR_VR * PR_MAX_TAPS];
  __shared__ __attribute__((aligned(16))) int bnd[2 * PR_VR];
  const PrImage im = tab.im[blockIdx.y];
  const int kh = im.kh, kv = im.kv, h_in = im.h_in, h_out = im.h_out, w_out = im.w_out;
  if (kv == 0 && kh != 0) return;                                    // the horizontal pass wrote the destination
  const int row_bytes = C * w_out;
  const unsigned tiles_x = (unsigned)(row_bytes + PR_VB - 1) / PR_VB, tiles_y = (unsigned)(h_out + PR_VR - 1) / PR_VR;
  if (blockIdx.x >= tiles_x * tiles_y) return;
  const int gb = (int)(blockIdx.x % tiles_x) * PR_VB + 4 * ((int)threadIdx.x & (PR_VB / 4 - 1));
  const int y0 = (int)(blockIdx.x / tiles_x) * PR_VR;
  const int ny = min(PR_VR, h_out - y0);
  const int tid = (int)threadIdx.x;
  if (kv != 0) {                                                     // the table h_in -> h_out follows the table w_in -> w_out
    const int* tb = reinterpret_cast<const int*>(tables + 16ull * im.tab16) + (kh != 0 ? w_out * (2 + kh) : 0);
    const int* tc = tb + 2 * h_out;
    for (int i = tid; i < 2 * ny; i += PR_THREADS) bnd[i] = tb[2 * y0 + i];
    for (int i = tid; i < ny * kv; i += PR_THREADS) kk[i] = tc[y0 * kv + i];
  }
  __syncthreads();
  if (gb >= row_bytes) return;
  const unsigned char* in = kh != 0 ? scratch + 16ull * im.scr16 : src + 16ull * im.src16;
  unsigned char* out = dst + 16ull * im.dst16;
  const bool dwords = (w_out & 3) == 0 && (ALIGNED || (((uintptr_t)in | (uintptr_t)out) & 3u) == 0);     // gb + 4 <= row_bytes then
  const int nbytes = min(4, row_bytes - gb);
  for (int r = tid / (PR_VB / 4); r < ny; r += PR_THREADS / (PR_VB / 4)) {
    const int yo = y0 + r;
    const int ymin = kv != 0 ? min(max(bnd[2 * r], 0), h_in - 1) : yo;
    const int count = kv != 0 ? max(min(min(bnd[2 * r + 1], kv), h_in - ymin), 0) : 1;
    const int* k = kk + r * kv;
    int acc[4] = {PR_HALF, PR_HALF, PR_HALF, PR_HALF};
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

// ------------------------------------------------------------------------------------------------ host
const char* size_problem(long long a, long long b) {
  if (a < 1 || b < 1 || a > PR_MAX_SIDE || b > PR_MAX_SIDE) return "bad size (every size is in 1 .. 16384)";
  return nullptr;
}

const char* axis_problem(long long in_size, long long out_size) {
  if (const char* problem = size_problem(in_size, out_size)) return problem;
  if (in_size > PR_MAX_RATIO * out_size || out_size > PR_MAX_RATIO * in_size) return "ratio out of range (at most 8 either way, per axis)";
  return nullptr;
}

const char* offset_problem(long long off) {
  if (off < 0 || off >= (1ll << 36)) return "offset outside [0, 2^36)";
  if ((off & 15) != 0) return "offset is not a multiple of 16";
  return nullptr;
}

// Everything after the entry's own argument checks: the checks of the buffers and of every record, the scratch and table accounting,
// the overlap check and the launches, 128 records at a time.  `name` is the entry, `things` what its records are ("images",
// "planes"); Rec is the entry's record (src_off, dst_off, tab_off, h_in, w_in, h_out, w_out) and ksize_of(record, horizontal) the
// ksize of one of its two tables; C, HW and ALIGNED are those of the two kernels.
template <int C, int HW, bool ALIGNED, typename Rec, typename KSize, typename HKernel, typename VKernel>
int pr_resize(const std::string& name, const std::string& things, const void* src, void* dst, const Rec* recs, int n, KSize ksize_of,
              const void* tables, long long tables_bytes, void* scratch, long long scratch_bytes, HKernel horizontal, VKernel vertical,
              hipStream_t st) {
  if (((uintptr_t)scratch & 15u) != 0) SRGD_EXT_FAIL(name + ": scratch must be 16-byte aligned");
  if (((uintptr_t)tables & 15u) != 0) SRGD_EXT_FAIL(name + ": tables must be 16-byte aligned");
  if (ALIGNED && (((uintptr_t)src | (uintptr_t)dst) & 15u) != 0) SRGD_EXT_FAIL(name + ": src and dst must be 16-byte aligned");
  const auto taps = [&](const Rec& im, bool h) { return (h ? im.w_in != im.w_out : im.h_in != im.h_out) ? (int)ksize_of(im, h) : 0; };
  long long scr = 0;
  Range s, d;
  for (int i = 0; i < n; ++i) {                          // every record is checked before the first launch
    const Rec& im = recs[i];
    const char* problem = axis_problem(im.h_in, im.h_out);
    if (!problem) problem = axis_problem(im.w_in, im.w_out);
    if (problem) SRGD_EXT_FAIL(name + ": " + problem);
    for (const long long off : {(long long)im.src_off, (long long)im.dst_off, (long long)im.tab_off}) {
      if (const char* p = offset_problem(off)) SRGD_EXT_FAIL(name + ": " + p);
    }
    const int kh = taps(im, true), kv = taps(im, false);
    if ((im.w_in != im.w_out && (kh < 1 || kh > PR_MAX_TAPS)) || (im.h_in != im.h_out && (kv < 1 || kv > PR_MAX_TAPS)))
      SRGD_EXT_FAIL(name + ": ksize outside 1 .. 49 (k_h, k_v: srgd_resize_ksize of the two tables)");
    const long long need = 4ll * (kh != 0 ? im.w_out * (2 + kh) : 0) + 4ll * (kv != 0 ? im.h_out * (2 + kv) : 0);      // bytes of the record's tables
    if (im.tab_off + need > tables_bytes) SRGD_EXT_FAIL(name + ": tables_bytes is too small for the " + things + "' tables");
    scr += round_up((long long)C * im.h_in * im.w_out, 16ll);
    s.add(im.src_off, (long long)C * im.h_in * im.w_in);
    d.add(im.dst_off, (long long)C * im.h_out * im.w_out);
  }
  if (scr > scratch_bytes)
    SRGD_EXT_FAIL(name + ": scratch_bytes is too small (sum of " + (C == 1 ? "" : std::to_string(C) + " * ") + "h_in * w_out, each rounded up to 16)");
  if (scr > (1ll << 36)) SRGD_EXT_FAIL(name + ": scratch beyond 2^36 bytes");
  if (s.meets(src, d, dst)) SRGD_EXT_FAIL(name + ": the source " + things + " and the destination " + things + " overlap");
  scr = 0;                                               // the records' scratch, packed in record order
  for (int first = 0; first < n; first += PR_MAX_IMAGES) {            // one launch sequence per PR_MAX_IMAGES records
    const int cnt = std::min(PR_MAX_IMAGES, n - first);
    PrTable tab;
    unsigned h_tiles = 0, v_tiles = 0;
    for (int k = 0; k < PR_MAX_IMAGES; ++k) tab.im[k] = PrImage{0u, 0u, 0u, 0u, 1, 1, 1, 1, 0, 0, 0, 0};
    for (int k = 0; k < cnt; ++k) {
      const Rec& im = recs[first + k];
      const int kh = taps(im, true), kv = taps(im, false);
      tab.im[k] = PrImage{(unsigned)(im.src_off >> 4), (unsigned)(im.dst_off >> 4), (unsigned)(scr >> 4), (unsigned)(im.tab_off >> 4),
                          (unsigned short)im.h_in, (unsigned short)im.w_in, (unsigned short)im.h_out, (unsigned short)im.w_out,
                          (unsigned char)kh, (unsigned char)kv, 0, 0};
      scr += round_up((long long)C * im.h_in * im.w_out, 16ll);
      if (kh != 0) h_tiles = std::max(h_tiles, (unsigned)((im.w_out + HW - 1) / HW) * (unsigned)((im.h_in + PR_HR - 1) / PR_HR));
      if (kv != 0 || kh == 0)
        v_tiles = std::max(v_tiles, (unsigned)((C * im.w_out + PR_VB - 1) / PR_VB) * (unsigned)((im.h_out + PR_VR - 1) / PR_VR));
    }
    if (h_tiles != 0)
      hipLaunchKernelGGL(horizontal, dim3(h_tiles, (unsigned)cnt), dim3(PR_THREADS), 0, st, tab, (const unsigned char*)src,
                         (unsigned char*)scratch, (unsigned char*)dst, (const unsigned char*)tables);
    if (v_tiles != 0)
      hipLaunchKernelGGL(vertical, dim3(v_tiles, (unsigned)cnt), dim3(PR_THREADS), 0, st, tab, (const unsigned char*)src,
                         (const unsigned char*)scratch, (unsigned char*)dst, (const unsigned char*)tables);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd
