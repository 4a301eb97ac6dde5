// Keeping the alpha channel of a transparent input on the GPU (engine extension, absent upstream): a Pillow-exact resize of 8-bit
// planes, the interleave of an RGB image and a plane into RGBA, and the spread of visible colours into the transparent area of an
// RGBA image.  The definitions are fixed in include/srgd_alpha.h.  All three are byte-moving, memory-bound integer kernels.
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument), blockIdx.x the tile.
//   plane resize, horizontal: the one-channel form of resize.hip's horizontal pass.  One workgroup of 256 threads per tile of 64
//               output pixels x 16 rows.  The tile's bounds and coefficient rows (at most 64 x 49 ints) and the bytes of its rows
//               between the first window's first pixel and the last window's end (at most 63 * 8 + 2 * 24 + 1 = 553 bytes, from the
//               dword in front of them) go to LDS; a thread owns one output pixel of rows r, r + 4, r + 8, r + 12: its coefficient
//               is read once per tap and serves four products; results go to LDS as bytes and leave as whole dwords along the row.
//   plane resize, vertical: resize.hip's vertical pass on rows of w bytes.  One workgroup per tile of 256 bytes x 16 output rows;
//               a thread owns dword j of the tile's rows r, r + 4, ...: every tap is one dword load along the contiguous byte axis
//               and four products with one coefficient, the result one dword store.  With no table at all (both passes skipped) the
//               same kernel copies: one tap of 2^22 at the output's own row.
//   pack:       an image is a flat run of h * w pixels, a thread owns 4 consecutive ones: three dword loads of colour, one of alpha,
//               one 16-byte store - aligned whatever w is, because the image bases are multiples of 16; the last h * w % 4 pixels
//               of an image are written one dword each from byte loads.
//   bleed:      one launch per pass, a thread per pixel of the dword state (R, G, B, known): a known pixel is copied, an unknown
//               one reads its 8 neighbours from the buffer of the pass before (the first pass reads the RGBA image itself: known is
//               "fourth byte > 0" in both).  A last kernel drops the fourth byte: a thread owns 4 pixels, one 16-byte load, three
//               dword stores.
// Rows of w bytes with w % 4 != 0 are not dword aligned: such planes take the guarded byte path of each resize kernel.
// Every index a kernel reads from a table is clamped to the plane and to the staged span before use, and every store is guarded by
// the sizes of the (host-checked) record: no table content can make a kernel read or write outside its plane.
// No atomics, no reductions: every byte depends on its own image alone - bit-identical alone, in any group, at any offset.
// LDS: horizontal 9,024 (rows) + 12,544 (coefficients) + 512 (bounds) + 1,024 (result) = 23,104 bytes; vertical 3,136 + 128.
#include <algorithm>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_alpha.h"
#include "ext_common.hpp"

// This file is a library of its own (libsrgd_alpha.so, include/srgd_alpha.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing.
namespace srgd {
namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_IMAGES = 128;                   // records travel as a kernel argument
constexpr int AL_MAX_TAPS = SRGD_ALPHA_MAX_TAPS;
constexpr int AL_HW = 64, AL_HR = 16;                // horizontal tile: output pixels x rows
constexpr int AL_HSPAN = 564;                        // LDS bytes of a staged source row: 141 dwords (odd: rows fall on different banks)
constexpr int AL_VB = 256, AL_VR = 16;               // vertical tile: bytes x output rows
static_assert((AL_HW - 1) * SRGD_ALPHA_MAX_RATIO + 2 * 3 * SRGD_ALPHA_MAX_RATIO + 1 + 3 + 3 <= AL_HSPAN && AL_HSPAN % 4 == 0,
              "the widest span of a tile, from the dword in front of it to the dword behind it, fits a staged row");
static_assert(AL_THREADS == AL_HW * (AL_HR / 4), "horizontal pass: a thread per output pixel and four rows");
static_assert(AL_THREADS == (AL_VB / 4) * 4 && AL_VR % 4 == 0, "vertical pass: a thread per dword, four rows at a time");
static_assert(2 * (int)(3 * SRGD_ALPHA_MAX_RATIO) + 1 == AL_MAX_TAPS, "lanczos at 8 : 1 is the widest table");

struct AlPlane {                                     // offsets in units of 16 bytes: [0, 2^36) bytes
  unsigned src16, dst16, scr16, tab16;
  unsigned short h_in, w_in, h_out, w_out;           // 1 .. 16384
  unsigned char kh, kv, pad0, pad1;                  // ksize of the two tables; 0: the pass is skipped
};
struct AlPlaneTable { AlPlane im[AL_MAX_IMAGES]; };
struct AlImage {                                     // pack: colour, plane, RGBA; bleed: RGBA source, RGB result, state buffer 0
  unsigned a16, b16, c16;
  unsigned short h, w;
};
struct AlImageTable { AlImage im[AL_MAX_IMAGES]; };
static_assert(sizeof(AlPlaneTable) <= 3584 && sizeof(AlImageTable) <= 3584, "the records and the pointers stay below 4 KiB of kernel arguments");

// Horizontal pass: src -> scratch (-> dst where the vertical pass is skipped).
__global__ __launch_bounds__(AL_THREADS) void alpha_plane_horizontal_kernel(AlPlaneTable tab, const unsigned char* __restrict__ src,
                                                                            unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                            const unsigned char* __restrict__ tables) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[AL_HR * AL_HSPAN];
  __shared__ __attribute__((aligned(16))) int kk[AL_HW * AL_MAX_TAPS];
  __shared__ __attribute__((aligned(16))) int bnd[2 * AL_HW];
  __shared__ __attribute__((aligned(16))) unsigned char res[AL_HR * AL_HW];
  const AlPlane im = tab.im[blockIdx.y];
  const int kh = im.kh, h_in = im.h_in, w_in = im.w_in, w_out = im.w_out;
  if (kh == 0) return;                                               // no horizontal pass for this plane
  const unsigned tiles_x = (unsigned)(w_out + AL_HW - 1) / AL_HW, tiles_y = (unsigned)(h_in + AL_HR - 1) / AL_HR;
  if (blockIdx.x >= tiles_x * tiles_y) return;                       // the grid is as wide as the launch's largest plane
  const int x0 = (int)(blockIdx.x % tiles_x) * AL_HW, y0 = (int)(blockIdx.x / tiles_x) * AL_HR;
  const int nx = min(AL_HW, w_out - x0), ny = min(AL_HR, h_in - y0);
  const int tid = (int)threadIdx.x;

  // 1. the tile's bounds and coefficient rows (the rows keep their stride kh, an odd number of dwords)
  const int* tb = reinterpret_cast<const int*>(tables + 16ull * im.tab16);
  const int* tc = tb + 2 * w_out;
  for (int i = tid; i < 2 * nx; i += AL_THREADS) bnd[i] = tb[2 * x0 + i];
  for (int i = tid; i < nx * kh; i += AL_THREADS) kk[i] = tc[x0 * kh + i];
  __syncthreads();

  // 2. the source span of the tile's rows: bytes [a0, a0 + span) of plane rows y0 .. y0 + ny - 1, a0 a multiple of 4 on the dword path
  const unsigned char* in = src + 16ull * im.src16;
  const bool in_dwords = (w_in & 3) == 0;                            // the base is a multiple of 16
  const int first = min(max(bnd[0], 0), w_in - 1);
  const int last_end = min(max(bnd[2 * (nx - 1)] + bnd[2 * (nx - 1) + 1], first), w_in);
  const int a0 = in_dwords ? (first & ~3) : first;
  const int span = min(last_end - a0, AL_HSPAN);                     // staged bytes of a row (<= 553 + 3 for every table within the ratio)
  if (in_dwords) {
    const int nd = (span + 3) >> 2;                                  // a0 + 4 nd <= w_in: both are multiples of 4 and a0 + span <= w_in
    for (int i = tid; i < ny * nd; i += AL_THREADS) {
      const int r = i / nd, d = i - r * nd;
      *reinterpret_cast<unsigned*>(rows + r * AL_HSPAN + 4 * d) =
          *reinterpret_cast<const unsigned*>(in + (size_t)(y0 + r) * (size_t)w_in + (size_t)(a0 + 4 * d));
    }
  } else {
    for (int i = tid; i < ny * span; i += AL_THREADS) {
      const int r = i / span, b = i - r * span;
      rows[r * AL_HSPAN + b] = in[(size_t)(y0 + r) * (size_t)w_in + (size_t)(a0 + b)];
    }
  }
  __syncthreads();

  // 3. output pixel x of the tile, rows rg, rg + 4, rg + 8, rg + 12 (rows beyond ny hold stale LDS bytes and are never stored)
  {
    const int x = tid & (AL_HW - 1), rg = tid / AL_HW;
    if (x < nx) {
      const int xmin = min(max(bnd[2 * x], first), w_in - 1);
      const int off = xmin - a0;                                     // >= 0
      const int count = max(min(min(bnd[2 * x + 1], kh), span - off), 0);            // every tap lies inside the staged span
      const unsigned char* p = rows + rg * AL_HSPAN + off;
      const int* k = kk + x * kh;
      int acc[4] = {1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1), 1 << (PILLOW_PREC_BITS - 1)};
      for (int t = 0; t < count; ++t) {
        const int kt = k[t];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += kt * (int)p[q * (AL_HR / 4) * AL_HSPAN + t];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) res[(rg + q * (AL_HR / 4)) * AL_HW + x] = (unsigned char)clip8(acc[q]);
    }
  }
  __syncthreads();

  // 4. the tile's result: bytes [x0, x0 + nx) of rows y0 .. y0 + ny - 1 of [h_in][w_out]
  unsigned char* out = im.kv == 0 ? dst + 16ull * im.dst16 : scratch + 16ull * im.scr16;
  if ((w_out & 3) == 0) {                                            // x0 = 64 tile and nx are multiples of 4 then
    const int nd = nx >> 2;
    for (int i = tid; i < ny * nd; i += AL_THREADS) {
      const int r = i / nd, d = i - r * nd;
      *reinterpret_cast<unsigned*>(out + (size_t)(y0 + r) * (size_t)w_out + (size_t)(x0 + 4 * d)) =
          *reinterpret_cast<const unsigned*>(res + r * AL_HW + 4 * d);
    }
  } else {
    for (int i = tid; i < ny * nx; i += AL_THREADS) {
      const int r = i / nx, b = i - r * nx;
      out[(size_t)(y0 + r) * (size_t)w_out + (size_t)(x0 + b)] = res[r * AL_HW + b];
    }
  }
}

// Vertical pass: scratch (src where the horizontal pass is skipped) -> dst; the copy where both are skipped.
__global__ __launch_bounds__(AL_THREADS) void alpha_plane_vertical_kernel(AlPlaneTable tab, const unsigned char* __restrict__ src,
                                                                          const unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                          const unsigned char* __restrict__ tables) {
  __shared__ __attribute__((aligned(16))) int kk[AL_VR * AL_MAX_TAPS];
  __shared__ __attribute__((aligned(16))) int bnd[2 * AL_VR];
  const AlPlane im = tab.im[blockIdx.y];
  const int kh = im.kh, kv = im.kv, h_in = im.h_in, h_out = im.h_out, w_out = im.w_out;
  if (kv == 0 && kh != 0) return;                                    // the horizontal pass wrote the destination
  const int row_bytes = w_out;
  const unsigned tiles_x = (unsigned)(row_bytes + AL_VB - 1) / AL_VB, tiles_y = (unsigned)(h_out + AL_VR - 1) / AL_VR;
  if (blockIdx.x >= tiles_x * tiles_y) return;
  const int gb = (int)(blockIdx.x % tiles_x) * AL_VB + 4 * ((int)threadIdx.x & (AL_VB / 4 - 1));
  const int y0 = (int)(blockIdx.x / tiles_x) * AL_VR;
  const int ny = min(AL_VR, h_out - y0);
  const int tid = (int)threadIdx.x;
  if (kv != 0) {                                                     // the table h_in -> h_out follows the table w_in -> w_out
    const int* tb = reinterpret_cast<const int*>(tables + 16ull * im.tab16) + (kh != 0 ? w_out * (2 + kh) : 0);
    const int* tc = tb + 2 * h_out;
    for (int i = tid; i < 2 * ny; i += AL_THREADS) bnd[i] = tb[2 * y0 + i];
    for (int i = tid; i < ny * kv; i += AL_THREADS) kk[i] = tc[y0 * kv + i];
  }
  __syncthreads();
  if (gb >= row_bytes) return;
  const unsigned char* in = kh != 0 ? scratch + 16ull * im.scr16 : src + 16ull * im.src16;
  unsigned char* out = dst + 16ull * im.dst16;
  const bool dwords = (w_out & 3) == 0;                              // gb + 4 <= row_bytes then; the bases are multiples of 16
  const int nbytes = min(4, row_bytes - gb);
  for (int r = tid / (AL_VB / 4); r < ny; r += AL_THREADS / (AL_VB / 4)) {
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

// Pack: a = colour [n][3], b = plane [n], c = RGBA [n][4]; thread q of an image owns pixels 4 q .. 4 q + 3.
__global__ __launch_bounds__(AL_THREADS) void alpha_pack_kernel(AlImageTable tab, const unsigned char* __restrict__ rgb,
                                                                const unsigned char* __restrict__ alpha, unsigned char* __restrict__ rgba) {
  const AlImage im = tab.im[blockIdx.y];
  const unsigned n = (unsigned)im.h * (unsigned)im.w;                // <= 2^28
  const unsigned q = blockIdx.x * AL_THREADS + threadIdx.x;          // < 2^26 + 256
  if (4u * q >= n) return;
  const unsigned char* c = rgb + 16ull * im.a16 + 12ull * q;
  const unsigned char* a = alpha + 16ull * im.b16 + 4ull * q;
  unsigned char* o = rgba + 16ull * im.c16 + 16ull * q;
  if (4u * q + 4u <= n) {
    const unsigned c0 = reinterpret_cast<const unsigned*>(c)[0], c1 = reinterpret_cast<const unsigned*>(c)[1],
                   c2 = reinterpret_cast<const unsigned*>(c)[2], aa = *reinterpret_cast<const unsigned*>(a);
    uint4 v;
    v.x = (c0 & 0x00ffffffu) | (aa << 24);
    v.y = (c0 >> 24) | ((c1 & 0x0000ffffu) << 8) | ((aa & 0x0000ff00u) << 16);
    v.z = (c1 >> 16) | ((c2 & 0x000000ffu) << 16) | ((aa & 0x00ff0000u) << 8);
    v.w = (c2 >> 8) | (aa & 0xff000000u);
    *reinterpret_cast<uint4*>(o) = v;
  } else {
    const unsigned rest = n - 4u * q;                                // 1 .. 3 pixels at the end of the image
    for (unsigned p = 0; p < rest; ++p)
      reinterpret_cast<unsigned*>(o)[p] = (unsigned)c[3 * p] | (unsigned)c[3 * p + 1] << 8 | (unsigned)c[3 * p + 2] << 16 | (unsigned)a[p] << 24;
  }
}

// One bleed pass: in -> out, both one dword per pixel (R, G, B, flag; known = flag > 0).  in is the RGBA image itself (first pass) or
// a state buffer; a16 / c16 of the record are the image's offsets in them.
__global__ __launch_bounds__(AL_THREADS) void alpha_bleed_pass_kernel(AlImageTable tab, const unsigned char* in_base, int in_is_source,
                                                                      unsigned char* out_base, unsigned long long in_shift16,
                                                                      unsigned long long out_shift16) {
  const AlImage im = tab.im[blockIdx.y];
  const int h = im.h, w = im.w;
  const unsigned n = (unsigned)h * (unsigned)w;
  const unsigned i = blockIdx.x * AL_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned* in = reinterpret_cast<const unsigned*>(in_base + 16ull * (in_is_source ? (unsigned long long)im.a16 : im.c16 + in_shift16));
  unsigned* out = reinterpret_cast<unsigned*>(out_base + 16ull * (im.c16 + out_shift16));
  const unsigned self = in[i];
  if ((self >> 24) != 0u) {                                          // known: never changes
    out[i] = self | 0xff000000u;
    return;
  }
  const int y = (int)(i / (unsigned)w), x = (int)(i - (unsigned)y * (unsigned)w);
  unsigned s0 = 0u, s1 = 0u, s2 = 0u, c = 0u;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if ((dy != 0 || dx != 0) && yy >= 0 && yy < h && xx >= 0 && xx < w) {
        const unsigned v = in[(size_t)yy * (size_t)w + (size_t)xx];
        if ((v >> 24) != 0u) {
          s0 += v & 0xffu;
          s1 += (v >> 8) & 0xffu;
          s2 += (v >> 16) & 0xffu;
          c += 1u;
        }
      }
    }
  }
  if (c == 0u) {
    out[i] = self;                                                   // still unknown: keeps its colour
    return;
  }
  out[i] = ((2u * s0 + c) / (2u * c)) | ((2u * s1 + c) / (2u * c)) << 8 | ((2u * s2 + c) / (2u * c)) << 16 | 0xff000000u;
}

// The end of a bleed: the first three bytes of every dword of `in` (the RGBA image itself where there was no pass) -> RGB; thread q
// of an image owns pixels 4 q .. 4 q + 3.
__global__ __launch_bounds__(AL_THREADS) void alpha_bleed_store_kernel(AlImageTable tab, const unsigned char* __restrict__ in_base, int in_is_source,
                                                                       unsigned long long in_shift16, unsigned char* __restrict__ rgb) {
  const AlImage im = tab.im[blockIdx.y];
  const unsigned n = (unsigned)im.h * (unsigned)im.w;
  const unsigned q = blockIdx.x * AL_THREADS + threadIdx.x;
  if (4u * q >= n) return;
  const unsigned char* s = in_base + 16ull * (in_is_source ? (unsigned long long)im.a16 : im.c16 + in_shift16) + 16ull * q;
  unsigned char* o = rgb + 16ull * im.b16 + 12ull * q;
  if (4u * q + 4u <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(s);
    reinterpret_cast<unsigned*>(o)[0] = (v.x & 0x00ffffffu) | (v.y << 24);
    reinterpret_cast<unsigned*>(o)[1] = ((v.y >> 8) & 0x0000ffffu) | (v.z << 16);
    reinterpret_cast<unsigned*>(o)[2] = ((v.z >> 16) & 0x000000ffu) | (v.w << 8);
  } else {
    const unsigned rest = n - 4u * q;
    for (unsigned p = 0; p < rest; ++p) {
      const unsigned v = reinterpret_cast<const unsigned*>(s)[p];
      o[3 * p] = (unsigned char)(v & 0xffu);
      o[3 * p + 1] = (unsigned char)((v >> 8) & 0xffu);
      o[3 * p + 2] = (unsigned char)((v >> 16) & 0xffu);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
const char* size_problem(long long a, long long b) {
  if (a < 1 || b < 1 || a > SRGD_ALPHA_MAX_SIDE || b > SRGD_ALPHA_MAX_SIDE) return "bad size (every size is in 1 .. 16384)";
  return nullptr;
}

const char* axis_problem(long long in_size, long long out_size) {
  if (const char* problem = size_problem(in_size, out_size)) return problem;
  if (in_size > SRGD_ALPHA_MAX_RATIO * out_size || out_size > SRGD_ALPHA_MAX_RATIO * in_size) return "ratio out of range (at most 8 either way, per axis)";
  return nullptr;
}

const char* offset_problem(long long off) {
  if (off < 0 || off >= (1ll << 36)) return "offset outside [0, 2^36)";
  if ((off & 15) != 0) return "offset is not a multiple of 16";
  return nullptr;
}

int resize_planes(const void* src, void* dst, const srgd_alpha_plane* planes, int n_planes, const void* tables, long long tables_bytes,
                  void* scratch, long long scratch_bytes, hipStream_t st) {
  const std::string name("srgd_alpha_resize_planes");
  if (n_planes < 1) SRGD_EXT_FAIL(name + ": n_planes must be >= 1");
  if (!src || !dst || !planes || !tables || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (((uintptr_t)scratch & 15u) != 0) SRGD_EXT_FAIL(name + ": scratch must be 16-byte aligned");
  if (((uintptr_t)tables & 15u) != 0) SRGD_EXT_FAIL(name + ": tables must be 16-byte aligned");
  if ((((uintptr_t)src | (uintptr_t)dst) & 15u) != 0) SRGD_EXT_FAIL(name + ": src and dst must be 16-byte aligned");
  long long scr = 0;
  Range s, d;
  for (int i = 0; i < n_planes; ++i) {                   // every plane is checked before the first launch
    const srgd_alpha_plane& im = planes[i];
    const char* problem = axis_problem(im.h_in, im.h_out);
    if (!problem) problem = axis_problem(im.w_in, im.w_out);
    if (problem) SRGD_EXT_FAIL(name + ": " + problem);
    for (const long long off : {(long long)im.src_off, (long long)im.dst_off, (long long)im.tab_off}) {
      if (const char* p = offset_problem(off)) SRGD_EXT_FAIL(name + ": " + p);
    }
    if ((im.w_in != im.w_out && (im.k_h < 1 || im.k_h > AL_MAX_TAPS)) || (im.h_in != im.h_out && (im.k_v < 1 || im.k_v > AL_MAX_TAPS)))
      SRGD_EXT_FAIL(name + ": ksize outside 1 .. 49 (k_h, k_v: srgd_resize_ksize of the two tables)");
    long long need = 0;                                  // bytes of the plane's tables
    if (im.w_in != im.w_out) need += 4ll * im.w_out * (2 + im.k_h);
    if (im.h_in != im.h_out) need += 4ll * im.h_out * (2 + im.k_v);
    if (im.tab_off + need > tables_bytes) SRGD_EXT_FAIL(name + ": tables_bytes is too small for the planes' tables");
    scr += round_up((long long)im.h_in * im.w_out, 16ll);
    s.add(im.src_off, (long long)im.h_in * im.w_in);
    d.add(im.dst_off, (long long)im.h_out * im.w_out);
  }
  if (scr > scratch_bytes) SRGD_EXT_FAIL(name + ": scratch_bytes is too small (sum of h_in * w_out, each rounded up to 16)");
  if (scr > (1ll << 36)) SRGD_EXT_FAIL(name + ": scratch beyond 2^36 bytes");
  if (s.meets(src, d, dst)) SRGD_EXT_FAIL(name + ": the source planes and the destination planes overlap");
  scr = 0;                                               // the planes' scratch, packed in plane order
  for (int first = 0; first < n_planes; first += AL_MAX_IMAGES) {     // one launch sequence per AL_MAX_IMAGES planes
    const int cnt = std::min(AL_MAX_IMAGES, n_planes - first);
    AlPlaneTable tab;
    unsigned h_tiles = 0, v_tiles = 0;
    for (int k = 0; k < AL_MAX_IMAGES; ++k) tab.im[k] = AlPlane{0u, 0u, 0u, 0u, 1, 1, 1, 1, 0, 0, 0, 0};
    for (int k = 0; k < cnt; ++k) {
      const srgd_alpha_plane& im = planes[first + k];
      const int kh = im.w_in != im.w_out ? im.k_h : 0, kv = im.h_in != im.h_out ? im.k_v : 0;
      tab.im[k] = AlPlane{(unsigned)(im.src_off >> 4), (unsigned)(im.dst_off >> 4), (unsigned)(scr >> 4), (unsigned)(im.tab_off >> 4),
                          (unsigned short)im.h_in, (unsigned short)im.w_in, (unsigned short)im.h_out, (unsigned short)im.w_out,
                          (unsigned char)kh, (unsigned char)kv, 0, 0};
      scr += round_up((long long)im.h_in * im.w_out, 16ll);
      if (kh != 0) h_tiles = std::max(h_tiles, (unsigned)((im.w_out + AL_HW - 1) / AL_HW) * (unsigned)((im.h_in + AL_HR - 1) / AL_HR));
      if (kv != 0 || kh == 0)
        v_tiles = std::max(v_tiles, (unsigned)((im.w_out + AL_VB - 1) / AL_VB) * (unsigned)((im.h_out + AL_VR - 1) / AL_VR));
    }
    if (h_tiles != 0)
      hipLaunchKernelGGL(alpha_plane_horizontal_kernel, dim3(h_tiles, (unsigned)cnt), dim3(AL_THREADS), 0, st, tab, (const unsigned char*)src,
                         (unsigned char*)scratch, (unsigned char*)dst, (const unsigned char*)tables);
    if (v_tiles != 0)
      hipLaunchKernelGGL(alpha_plane_vertical_kernel, dim3(v_tiles, (unsigned)cnt), dim3(AL_THREADS), 0, st, tab, (const unsigned char*)src,
                         (const unsigned char*)scratch, (unsigned char*)dst, (const unsigned char*)tables);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

int pack_rgba(const void* rgb, const void* alpha, void* rgba, const srgd_alpha_image* images, int n_images, hipStream_t st) {
  const std::string name("srgd_alpha_pack_rgba");
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!rgb || !alpha || !rgba || !images) SRGD_EXT_FAIL(name + ": null argument");
  if ((((uintptr_t)rgb | (uintptr_t)alpha | (uintptr_t)rgba) & 15u) != 0) SRGD_EXT_FAIL(name + ": rgb, alpha and rgba must be 16-byte aligned");
  Range c, a, d;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const srgd_alpha_image& im = images[i];
    if (const char* problem = size_problem(im.h, im.w)) SRGD_EXT_FAIL(name + ": " + problem);
    for (const long long off : {(long long)im.rgb_off, (long long)im.a_off, (long long)im.rgba_off}) {
      if (const char* p = offset_problem(off)) SRGD_EXT_FAIL(name + ": " + p);
    }
    const long long n = (long long)im.h * im.w;
    c.add(im.rgb_off, 3 * n);
    a.add(im.a_off, n);
    d.add(im.rgba_off, 4 * n);
  }
  if (d.meets(rgba, c, rgb) || d.meets(rgba, a, alpha)) SRGD_EXT_FAIL(name + ": the destination images overlap the colour or the planes");
  for (int first = 0; first < n_images; first += AL_MAX_IMAGES) {
    const int cnt = std::min(AL_MAX_IMAGES, n_images - first);
    AlImageTable tab;
    unsigned blocks = 0;
    for (int k = 0; k < AL_MAX_IMAGES; ++k) tab.im[k] = AlImage{0u, 0u, 0u, 1, 1};
    for (int k = 0; k < cnt; ++k) {
      const srgd_alpha_image& im = images[first + k];
      tab.im[k] = AlImage{(unsigned)(im.rgb_off >> 4), (unsigned)(im.a_off >> 4), (unsigned)(im.rgba_off >> 4), (unsigned short)im.h,
                          (unsigned short)im.w};
      const long long quads = ((long long)im.h * im.w + 3) / 4;
      blocks = std::max(blocks, (unsigned)((quads + AL_THREADS - 1) / AL_THREADS));
    }
    hipLaunchKernelGGL(alpha_pack_kernel, dim3(blocks, (unsigned)cnt), dim3(AL_THREADS), 0, st, tab, (const unsigned char*)rgb,
                       (const unsigned char*)alpha, (unsigned char*)rgba);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

int bleed(const void* rgba, void* rgb, const srgd_alpha_image* images, int n_images, int passes, void* scratch, long long scratch_bytes,
          hipStream_t st) {
  const std::string name("srgd_alpha_bleed");
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!rgba || !rgb || !images || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (passes < 0 || passes > SRGD_ALPHA_MAX_BLEED) SRGD_EXT_FAIL(name + ": passes must be in 0 .. 64");
  if (((uintptr_t)scratch & 15u) != 0) SRGD_EXT_FAIL(name + ": scratch must be 16-byte aligned");
  if ((((uintptr_t)rgba | (uintptr_t)rgb) & 15u) != 0) SRGD_EXT_FAIL(name + ": rgba and rgb must be 16-byte aligned");
  long long state = 0;                                   // bytes of one of the two state buffers
  Range s, d;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const srgd_alpha_image& im = images[i];
    if (const char* problem = size_problem(im.h, im.w)) SRGD_EXT_FAIL(name + ": " + problem);
    for (const long long off : {(long long)im.rgb_off, (long long)im.rgba_off}) {
      if (const char* p = offset_problem(off)) SRGD_EXT_FAIL(name + ": " + p);
    }
    const long long n = (long long)im.h * im.w;
    state += round_up(4 * n, 16ll);
    s.add(im.rgba_off, 4 * n);
    d.add(im.rgb_off, 3 * n);
  }
  if (passes > 0 && 2 * state > scratch_bytes) SRGD_EXT_FAIL(name + ": scratch_bytes is too small (twice the sum of 4 * h * w, each rounded up to 16)");
  if (2 * state > (1ll << 36)) SRGD_EXT_FAIL(name + ": scratch beyond 2^36 bytes");
  if (s.meets(rgba, d, rgb)) SRGD_EXT_FAIL(name + ": the source images and the destination images overlap");
  const unsigned long long state16 = (unsigned long long)(state >> 4);
  long long scr = 0;                                     // the images' state, packed in image order in each of the two buffers
  for (int first = 0; first < n_images; first += AL_MAX_IMAGES) {
    const int cnt = std::min(AL_MAX_IMAGES, n_images - first);
    AlImageTable tab;
    unsigned pixel_blocks = 0, quad_blocks = 0;
    for (int k = 0; k < AL_MAX_IMAGES; ++k) tab.im[k] = AlImage{0u, 0u, 0u, 1, 1};
    for (int k = 0; k < cnt; ++k) {
      const srgd_alpha_image& im = images[first + k];
      const long long n = (long long)im.h * im.w;
      tab.im[k] = AlImage{(unsigned)(im.rgba_off >> 4), (unsigned)(im.rgb_off >> 4), (unsigned)(scr >> 4), (unsigned short)im.h,
                          (unsigned short)im.w};
      scr += round_up(4 * n, 16ll);
      pixel_blocks = std::max(pixel_blocks, (unsigned)((n + AL_THREADS - 1) / AL_THREADS));
      quad_blocks = std::max(quad_blocks, (unsigned)(((n + 3) / 4 + AL_THREADS - 1) / AL_THREADS));
    }
    for (int p = 0; p < passes; ++p)                     // pass p: buffer (p - 1) & 1 (the source for p = 0) -> buffer p & 1
      hipLaunchKernelGGL(alpha_bleed_pass_kernel, dim3(pixel_blocks, (unsigned)cnt), dim3(AL_THREADS), 0, st, tab,
                         p == 0 ? (const unsigned char*)rgba : (const unsigned char*)scratch, p == 0 ? 1 : 0, (unsigned char*)scratch,
                         ((p - 1) & 1) ? state16 : 0ull, (p & 1) ? state16 : 0ull);
    hipLaunchKernelGGL(alpha_bleed_store_kernel, dim3(quad_blocks, (unsigned)cnt), dim3(AL_THREADS), 0, st, tab,
                       passes == 0 ? (const unsigned char*)rgba : (const unsigned char*)scratch, passes == 0 ? 1 : 0,
                       ((passes - 1) & 1) ? state16 : 0ull, (unsigned char*)rgb);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_alpha_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_alpha_resize_planes(const void* src, void* dst, const srgd_alpha_plane* planes_host, int n_planes, const void* tables,
                                             int64_t tables_bytes, void* scratch, int64_t scratch_bytes, void* stream) {
  return resize_planes(src, dst, planes_host, n_planes, tables, (long long)tables_bytes, scratch, (long long)scratch_bytes, (hipStream_t)stream);
}

SRGD_EXT_EXPORT int srgd_alpha_pack_rgba(const void* rgb, const void* alpha, void* rgba, const srgd_alpha_image* images_host, int n_images,
                                         void* stream) {
  return pack_rgba(rgb, alpha, rgba, images_host, n_images, (hipStream_t)stream);
}

SRGD_EXT_EXPORT int srgd_alpha_bleed(const void* rgba, void* rgb, const srgd_alpha_image* images_host, int n_images, int passes, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
  return bleed(rgba, rgb, images_host, n_images, passes, scratch, (long long)scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
