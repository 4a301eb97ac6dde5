// Keeping the alpha channel of a transparent input on the GPU (engine extension, absent upstream): a Pillow-exact resize of 8-bit
// planes, the interleave of an RGB image and a plane into RGBA, and the spread of visible colours into the transparent area of an
// RGBA image.  The definitions are fixed in include/srgd_alpha.h.  All three are byte-moving, memory-bound integer kernels.
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument), blockIdx.x the tile.
//   plane resize: the two passes and the host driver of pillow_resample.hpp (shared with resize.hip, as a header), instantiated for 1
//               channel, a horizontal tile of 64 output pixels x 16 rows and four rows per thread (rows r, r + 4, r + 8, r + 12: a
//               coefficient serves four products), and bases that the host has checked to 16 bytes.
//   pack:       an image is a flat run of h * w pixels, a thread owns 4 consecutive ones: three dword loads of colour, one of alpha,
//               one 16-byte store - aligned whatever w is, because the image bases are multiples of 16; the last h * w % 4 pixels
//               of an image are written one dword each from byte loads.
//   bleed:      one launch per pass, a thread per pixel of the dword state (R, G, B, known): a known pixel is copied, an unknown
//               one reads its 8 neighbours from the buffer of the pass before (the first pass reads the RGBA image itself: known is
//               "fourth byte > 0" in both).  A last kernel drops the fourth byte: a thread owns 4 pixels, one 16-byte load, three
//               dword stores.
// Rows of w bytes with w % 4 != 0 are not dword aligned: such planes take the guarded byte path of each resize kernel.
// No atomics, no reductions: every byte depends on its own image alone - bit-identical alone, in any group, at any offset.
// LDS: horizontal 9,024 (rows) + 12,544 (coefficients) + 512 (bounds) + 1,024 (result) = 23,104 bytes; vertical 3,136 + 128.
#include <algorithm>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_alpha.h"
#include "pillow_resample.hpp"

// This file is a library of its own (libsrgd_alpha.so, include/srgd_alpha.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing, pillow_resample.hpp the resize it has in common with resize.hip.
namespace srgd {
namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_IMAGES = 128;                   // records travel as a kernel argument
constexpr int AL_HW = 64, AL_R = 4;                  // horizontal tile: 64 output pixels x 16 rows, four rows per thread
static_assert(PR_MAX_SIDE == SRGD_ALPHA_MAX_SIDE && PR_MAX_RATIO == SRGD_ALPHA_MAX_RATIO && PR_MAX_TAPS == SRGD_ALPHA_MAX_TAPS,
              "the limits of include/srgd_alpha.h");

struct AlImage {                                     // pack: colour, plane, RGBA; bleed: RGBA source, RGB result, state buffer 0
  unsigned a16, b16, c16;
  unsigned short h, w;
};
struct AlImageTable { AlImage im[AL_MAX_IMAGES]; };
static_assert(sizeof(AlImageTable) <= 3584, "the records and the pointers stay below 4 KiB of kernel arguments");

__global__ __launch_bounds__(PR_THREADS) void alpha_plane_horizontal_kernel(PrTable tab, const unsigned char* __restrict__ src,
                                                                            unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                            const unsigned char* __restrict__ tables) {
  pr_horizontal<1, AL_HW, AL_R, true>(tab, src, scratch, dst, tables);
}

__global__ __launch_bounds__(PR_THREADS) void alpha_plane_vertical_kernel(PrTable tab, const unsigned char* __restrict__ src,
                                                                          const unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst,
                                                                          const unsigned char* __restrict__ tables) {
  pr_vertical<1, true>(tab, src, scratch, dst, tables);
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
int resize_planes(const void* src, void* dst, const srgd_alpha_plane* planes, int n_planes, const void* tables, long long tables_bytes,
                  void* scratch, long long scratch_bytes, hipStream_t st) {
  const std::string name("srgd_alpha_resize_planes");
  if (n_planes < 1) SRGD_EXT_FAIL(name + ": n_planes must be >= 1");
  if (!src || !dst || !planes || !tables || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  const auto ksize_of = [](const srgd_alpha_plane& im, bool h) { return h ? im.k_h : im.k_v; };
  return pr_resize<1, AL_HW, true>(name, "planes", src, dst, planes, n_planes, ksize_of, tables, tables_bytes, scratch, scratch_bytes,
                                   alpha_plane_horizontal_kernel, alpha_plane_vertical_kernel, st);
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
