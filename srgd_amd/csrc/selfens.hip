// Geometric self-ensemble on the GPU (engine extension, absent upstream): the eight dihedral operations on 8-bit RGB images and the
// fused "turn every source back and average".  The definitions are fixed in include/srgd_selfens.h.  Both entries are byte-moving,
// memory-bound integer kernels and share one tile routine: the transform is the merge of ONE source whose op is the inverse of the
// asked one (m = (2 S + 1) div 2 = S).
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument), blockIdx.x the tile of 32 x 32 output pixels; 256
// threads.  Per source the record holds "gather flags": bit 2 = output (y, x) reads source (row, column) from (x, y) instead of
// (y, x), bit 1 = the source row index is reversed, bit 0 = the source column index is reversed.  For a merge the flags of source j
// are op_j itself; for a transform they are inverse(op).
//   stage:   the tile's rectangle of every source - 32 rows of at most 96 bytes - goes to LDS.  Thread t owns the 16-byte aligned
//            slot t % 7 of source row t / 7 (7 slots cover 15 bytes of phase + 96 bytes): a slot wholly inside the run is one
//            16-byte load and four dword LDS writes, a slot the run starts or ends in is copied byte by byte, so no byte outside the
//            run is read.  An LDS row keeps the run's phase modulo 16 and has a stride of 116 bytes = 29 dwords (odd: the column
//            walks of a transposing op fall on different banks).
//   sum:     thread t owns the 16-byte aligned slot t % 7 of output row t / 7.  Its 16 bytes touch at most 6 pixels; per pixel and
//            source one LDS address (row, phase, column) and three byte reads, summed in 32-bit registers per (pixel, channel); the
//            slot's bytes are then picked by the slot's channel phase, m = ((2 S + n) * magic) >> 20 with magic = 2^20 div 2n + 1
//            (exact for S <= 2040, n <= 8: checked at compile time below), one 16-byte store, or byte stores where the row starts
//            or ends inside the slot.
//   mean01:  the merged bytes also go to a 32 x 96 byte LDS tile; after a barrier, thread t walks the slots of 4 floats of the three
//            planes' rows: (float)m / 255.0f, one 16-byte store where the slot lies inside the run, single floats at its ends.
// No atomics, no reductions: every byte depends on its own image alone - bit-identical alone, in any group, at any offset.
// LDS: transform 3,712 bytes (one source tile), merge 8 x 3,712 + 3,072 = 32,768 bytes.
#include <algorithm>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_selfens.h"
#include "ext_common.hpp"

// This file is a library of its own (libsrgd_selfens.so, include/srgd_selfens.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing (pillow_resample.hpp and pillow_x4.hpp, the code some of them have in
// common, are headers too: no symbol is shared).
namespace srgd {
namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_MAX_IMAGES = SRGD_SELFENS_MAX_IMAGES;       // records travel as a kernel argument
constexpr int SE_MAX_SOURCES = SRGD_SELFENS_MAX_SOURCES;
constexpr int SE_TILE = SRGD_SELFENS_TILE;                   // output pixels per side of a tile
constexpr int SE_RUN = 3 * SE_TILE;                          // bytes of a tile's row
constexpr int SE_SLOTS = (15 + SE_RUN + 15) / 16;            // 16-byte aligned slots that a run of any phase can touch: 7
constexpr int SE_STRIDE = 116;                               // LDS bytes of a staged source row
constexpr int SE_SRC_TILE = SE_TILE * SE_STRIDE;             // LDS bytes of one source's tile
constexpr int SE_FSLOTS = (3 + SE_TILE + 3) / 4;             // slots of 4 floats that a plane row's run of any phase can touch: 9
constexpr int SE_MAGIC_SHIFT = 20;
static_assert(SE_SLOTS * SE_TILE <= SE_THREADS, "a thread per slot of the tile");
static_assert(SE_STRIDE % 4 == 0 && (SE_STRIDE / 4) % 2 == 1 && SE_STRIDE >= 16 * SE_SLOTS && SE_STRIDE >= 15 + SE_RUN, "a staged row");
static_assert(SE_SRC_TILE == SRGD_SELFENS_LDS_SOURCE && SE_SRC_TILE == SRGD_SELFENS_LDS_TRANSFORM &&
                  SE_MAX_SOURCES * SE_SRC_TILE + SE_TILE * SE_RUN == SRGD_SELFENS_LDS_MERGE,
              "the header states the LDS sizes");

constexpr unsigned se_magic(int n) { return (1u << SE_MAGIC_SHIFT) / (2u * (unsigned)n) + 1u; }
constexpr bool se_magic_is_exact() {
  for (int n = 1; n <= SE_MAX_SOURCES; ++n)
    for (unsigned s = 0; s <= 255u * (unsigned)n; ++s)
      if ((((2u * s + (unsigned)n) * se_magic(n)) >> SE_MAGIC_SHIFT) != (2u * s + (unsigned)n) / (2u * (unsigned)n)) return false;
  return true;
}
static_assert(se_magic_is_exact(), "the multiply-shift is the integer division of the definition for every sum that can occur");

struct SeSource {
  unsigned off16;                                    // offset in units of 16 bytes: [0, 2^36) bytes
  unsigned flags;                                    // gather flags: 4 = exchange (y, x), 2 = reverse the source rows, 1 = the columns
};
template <int NS>
struct SeImage {
  unsigned dst16;
  int H, W, n;                                       // output size; sources
  unsigned magic, pad;
  unsigned long long m01;                            // first element of the image's planes in mean01
  SeSource s[NS];
};
template <int NS>
struct SeTable { SeImage<NS> im[SE_MAX_IMAGES]; };
static_assert(sizeof(SeTable<SE_MAX_SOURCES>) <= 3584, "the records and the pointers stay below 4 KiB of kernel arguments");

// The rectangle of a source that a tile of the output reads: nrows runs of 3 * ncols bytes, run i from byte g0 + i * rs of the source.
struct SeGeo {
  int nrows, ncols;
  unsigned rs, g0;
  bool t, fr, fc;
};
__device__ __forceinline__ SeGeo se_geo(unsigned flags, int H, int W, int x0, int y0, int nx, int ny) {
  SeGeo g;
  g.t = (flags & 4u) != 0;
  g.fr = (flags & 2u) != 0;
  g.fc = (flags & 1u) != 0;
  const int sh = g.t ? W : H, sw = g.t ? H : W;
  g.nrows = g.t ? nx : ny;
  g.ncols = g.t ? ny : nx;
  const int r00 = g.t ? x0 : y0, c00 = g.t ? y0 : x0;
  const int rlo = g.fr ? sh - r00 - g.nrows : r00, clo = g.fc ? sw - c00 - g.ncols : c00;
  g.rs = 3u * (unsigned)sw;
  g.g0 = (unsigned)rlo * g.rs + 3u * (unsigned)clo;  // < 3 * h * w < 2^31
  return g;
}

template <int NS, bool MEAN>
__device__ __forceinline__ void se_tile(const SeImage<NS>& im, const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                        float* __restrict__ mean01, unsigned char* tiles, unsigned char* mtile) {
  const int H = im.H, W = im.W, n = im.n;
  const unsigned tiles_x = (unsigned)(W + SE_TILE - 1) / SE_TILE, tiles_y = (unsigned)(H + SE_TILE - 1) / SE_TILE;
  if (blockIdx.x >= tiles_x * tiles_y) return;                       // the grid is as wide as the launch's largest image
  const int x0 = (int)(blockIdx.x % tiles_x) * SE_TILE, y0 = (int)(blockIdx.x / tiles_x) * SE_TILE;
  const int nx = min(SE_TILE, W - x0), ny = min(SE_TILE, H - y0);
  const int tid = (int)threadIdx.x;
  const int row = tid / SE_SLOTS, q = tid - SE_SLOTS * row;          // the thread's slot, of a source row and of an output row

  // 1. stage: the tile's rectangle of every source
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    if (j < n) {
      const SeGeo g = se_geo(im.s[j].flags, H, W, x0, y0, nx, ny);
      if (row < g.nrows) {
        const unsigned gs = g.g0 + (unsigned)row * g.rs;             // the run: bytes [gs, gs + 3 ncols) of the source
        const unsigned cb = (gs & ~15u) + 16u * (unsigned)q;         // the slot: bytes [cb, cb + 16)
        const unsigned lo = max(cb, gs), hi = min(cb + 16u, gs + 3u * (unsigned)g.ncols);
        if (hi > lo) {
          const unsigned char* p = src + 16ull * im.s[j].off16 + cb;
          unsigned char* t = tiles + j * SE_SRC_TILE + row * SE_STRIDE + 16 * q;
          if (hi - lo == 16u) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            reinterpret_cast<unsigned*>(t)[0] = v.x;
            reinterpret_cast<unsigned*>(t)[1] = v.y;
            reinterpret_cast<unsigned*>(t)[2] = v.z;
            reinterpret_cast<unsigned*>(t)[3] = v.w;
          } else {
            for (unsigned b = lo - cb; b < hi - cb; ++b) t[b] = p[b];
          }
        }
      }
    }
  }
  __syncthreads();

  // 2. sum: slot q of output row y0 + row
  if (row < ny) {
    const unsigned ds = (unsigned)(y0 + row) * 3u * (unsigned)W + 3u * (unsigned)x0;     // the run: bytes [ds, ds + 3 nx) of the output
    const unsigned cb = (ds & ~15u) + 16u * (unsigned)q;
    const unsigned lo = max(cb, ds), hi = min(cb + 16u, ds + 3u * (unsigned)nx);
    if (hi > lo) {
      const int k0 = (int)cb - (int)ds;                              // byte b of the slot is byte k0 + b of the run; >= -15
      const int pxf = (k0 + 18) / 3 - 6;                             // floor(k0 / 3): the pixel of the slot's first byte
      const int off = k0 - 3 * pxf;                                  // its channel: 0, 1, 2
      unsigned s[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) s[i] = 0u;
      for (int j = 0; j < n; ++j) {
        const SeGeo g = se_geo(im.s[j].flags, H, W, x0, y0, nx, ny);
        const unsigned char* tile = tiles + j * SE_SRC_TILE;
#pragma unroll
        for (int pp = 0; pp < 6; ++pp) {
          const int px = pxf + pp;
          if (px >= 0 && px < nx) {
            const int r0 = g.t ? px : row, c0 = g.t ? row : px;
            const int i = g.fr ? g.nrows - 1 - r0 : r0, c = g.fc ? g.ncols - 1 - c0 : c0;
            const unsigned char* p = tile + i * SE_STRIDE + (int)((g.g0 + (unsigned)i * g.rs) & 15u) + 3 * c;
            s[3 * pp] += p[0];
            s[3 * pp + 1] += p[1];
            s[3 * pp + 2] += p[2];
          }
        }
      }
      unsigned m[16];
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const unsigned v = off == 0 ? s[b] : (off == 1 ? s[b + 1] : s[b + 2]);
        m[b] = ((2u * v + (unsigned)n) * im.magic) >> SE_MAGIC_SHIFT;
      }
      unsigned char* o = dst + 16ull * im.dst16 + cb;
      if (hi - lo == 16u) {
        uint4 v;
        v.x = m[0] | m[1] << 8 | m[2] << 16 | m[3] << 24;
        v.y = m[4] | m[5] << 8 | m[6] << 16 | m[7] << 24;
        v.z = m[8] | m[9] << 8 | m[10] << 16 | m[11] << 24;
        v.w = m[12] | m[13] << 8 | m[14] << 16 | m[15] << 24;
        *reinterpret_cast<uint4*>(o) = v;
      } else {
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          if ((unsigned)b >= lo - cb && (unsigned)b < hi - cb) o[b] = (unsigned char)m[b];
        }
      }
      if (MEAN && mean01 != nullptr) {
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          if ((unsigned)b >= lo - cb && (unsigned)b < hi - cb) mtile[row * SE_RUN + k0 + b] = (unsigned char)m[b];
        }
      }
    }
  }

  // 3. mean01: the three planes' rows of the tile, slots of 4 floats
  if (MEAN && mean01 != nullptr) {                                   // the same in every thread of the launch
    __syncthreads();
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    const unsigned long long base = ((unsigned long long)reinterpret_cast<uintptr_t>(mean01) >> 2) + im.m01;      // in floats
    for (int it = tid; it < 3 * SE_TILE * SE_FSLOTS; it += SE_THREADS) {
      const int ch = it / (SE_TILE * SE_FSLOTS), rem = it - ch * (SE_TILE * SE_FSLOTS);
      const int yy = rem / SE_FSLOTS, qq = rem - yy * SE_FSLOTS;
      if (yy < ny) {
        const unsigned long long e = base + (unsigned long long)ch * hw + (unsigned long long)(y0 + yy) * (unsigned long long)W +
                                     (unsigned long long)x0;        // the run: floats [e, e + nx)
        const unsigned long long cb = (e & ~3ull) + 4ull * (unsigned long long)qq;
        const unsigned long long lo = max(cb, e), hi = min(cb + 4ull, e + (unsigned long long)nx);
        if (hi > lo) {
          const int p0 = (int)((long long)cb - (long long)e);        // float p of the slot is pixel p0 + p of the tile's row; >= -3
          const unsigned char* mrow = mtile + yy * SE_RUN + ch;
          float* o = reinterpret_cast<float*>(static_cast<uintptr_t>(cb << 2));
          if (hi - lo == 4ull) {
            float4 f;
            f.x = (float)mrow[3 * p0] / 255.0f;
            f.y = (float)mrow[3 * (p0 + 1)] / 255.0f;
            f.z = (float)mrow[3 * (p0 + 2)] / 255.0f;
            f.w = (float)mrow[3 * (p0 + 3)] / 255.0f;
            *reinterpret_cast<float4*>(o) = f;
          } else {
            for (int p = (int)(lo - cb); p < (int)(hi - cb); ++p) o[p] = (float)mrow[3 * (p0 + p)] / 255.0f;
          }
        }
      }
    }
  }
}

// dst = apply(src, op): one source per image, its gather flags are inverse(op).
__global__ __launch_bounds__(SE_THREADS) void selfens_transform_kernel(SeTable<1> tab, const unsigned char* __restrict__ src,
                                                                       unsigned char* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) unsigned char tiles[SE_SRC_TILE];
  se_tile<1, false>(tab.im[blockIdx.y], src, dst, nullptr, tiles, nullptr);
}

// The merge: up to eight sources per image, turned back and averaged; mean01 where it is not null.
__global__ __launch_bounds__(SE_THREADS) void selfens_merge_kernel(SeTable<SE_MAX_SOURCES> tab, const unsigned char* __restrict__ src,
                                                                   unsigned char* __restrict__ dst, float* __restrict__ mean01) {
  __shared__ __attribute__((aligned(16))) unsigned char tiles[SE_MAX_SOURCES * SE_SRC_TILE];
  __shared__ __attribute__((aligned(16))) unsigned char mtile[SE_TILE * SE_RUN];
  se_tile<SE_MAX_SOURCES, true>(tab.im[blockIdx.y], src, dst, mean01, tiles, mtile);
}

// ------------------------------------------------------------------------------------------------ host
const char* size_problem(long long h, long long w) {
  if (h < 1 || w < 1) return "bad size (h and w are >= 1)";
  // with both sides >= 1 neither can reach 2^31 / 3: checked first, so that the product below stays far inside 64 bits
  if (h > (1ll << 31) / 3 || w > (1ll << 31) / 3 || 3 * h * w >= (1ll << 31)) return "bad size (3*h*w must be < 2^31)";
  return nullptr;
}

const char* offset_problem(long long off) {
  if (off < 0 || off >= (1ll << 36)) return "offset outside [0, 2^36)";
  if ((off & 15) != 0) return "offset is not a multiple of 16";
  return nullptr;
}

constexpr int inverse_op(int op) { return op == 5 ? 6 : (op == 6 ? 5 : op); }

unsigned tiles_of(long long h, long long w) { return (unsigned)(((h + SE_TILE - 1) / SE_TILE) * ((w + SE_TILE - 1) / SE_TILE)); }

int transform(const void* src, void* dst, const srgd_selfens_record* records, int n, hipStream_t st) {
  const std::string name("srgd_selfens_transform");
  if (n < 1) SRGD_EXT_FAIL(name + ": n must be >= 1");
  if (!src || !dst || !records) SRGD_EXT_FAIL(name + ": null argument");
  if ((((uintptr_t)src | (uintptr_t)dst) & 15u) != 0) SRGD_EXT_FAIL(name + ": src and dst must be 16-byte aligned");
  Range s, d;
  for (int i = 0; i < n; ++i) {                          // every image is checked before the first launch
    const srgd_selfens_record& r = records[i];
    if (const char* problem = size_problem(r.h, r.w)) SRGD_EXT_FAIL(name + ": " + problem);
    if (r.op < 0 || r.op > 7) SRGD_EXT_FAIL(name + ": op outside 0 .. 7");
    for (const long long off : {(long long)r.src_off, (long long)r.dst_off}) {
      if (const char* p = offset_problem(off)) SRGD_EXT_FAIL(name + ": " + p);
    }
    s.add(r.src_off, 3ll * r.h * r.w);
    d.add(r.dst_off, 3ll * r.h * r.w);
  }
  if (s.meets(src, d, dst)) SRGD_EXT_FAIL(name + ": the source images and the destination images overlap");
  for (int first = 0; first < n; first += SE_MAX_IMAGES) {            // one launch per SE_MAX_IMAGES images
    const int cnt = std::min(SE_MAX_IMAGES, n - first);
    SeTable<1> tab;
    unsigned blocks = 0;
    for (int k = 0; k < SE_MAX_IMAGES; ++k) tab.im[k] = SeImage<1>{0u, 1, 1, 1, se_magic(1), 0u, 0ull, {{0u, 0u}}};
    for (int k = 0; k < cnt; ++k) {
      const srgd_selfens_record& r = records[first + k];
      const bool t = (r.op & 4) != 0;                    // the output is [w][h][3] then
      tab.im[k] = SeImage<1>{(unsigned)(r.dst_off >> 4), t ? r.w : r.h, t ? r.h : r.w, 1, se_magic(1), 0u, 0ull,
                             {{(unsigned)(r.src_off >> 4), (unsigned)inverse_op(r.op)}}};
      blocks = std::max(blocks, tiles_of(r.h, r.w));
    }
    hipLaunchKernelGGL(selfens_transform_kernel, dim3(blocks, (unsigned)cnt), dim3(SE_THREADS), 0, st, tab, (const unsigned char*)src,
                       (unsigned char*)dst);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

int merge(const void* src, void* dst, float* mean01, const srgd_selfens_image* images, int n_images, hipStream_t st) {
  const std::string name("srgd_selfens_merge");
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!src || !dst || !images) SRGD_EXT_FAIL(name + ": null argument");
  if ((((uintptr_t)src | (uintptr_t)dst) & 15u) != 0) SRGD_EXT_FAIL(name + ": src and dst_u8 must be 16-byte aligned");
  if (((uintptr_t)mean01 & 3u) != 0) SRGD_EXT_FAIL(name + ": mean01 must be 4-byte aligned");
  Range s, d;
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const srgd_selfens_image& im = images[i];
    if (im.n_src < 1 || im.n_src > SE_MAX_SOURCES) SRGD_EXT_FAIL(name + ": n_src outside 1 .. 8");
    if (const char* problem = size_problem(im.H, im.W)) SRGD_EXT_FAIL(name + ": " + problem);
    if (const char* p = offset_problem(im.dst_off)) SRGD_EXT_FAIL(name + ": " + p);
    if (mean01 && im.mean01_off < 0) SRGD_EXT_FAIL(name + ": negative mean01 offset");
    if (mean01 && im.mean01_off >= (1ll << 40)) SRGD_EXT_FAIL(name + ": mean01 offset beyond 2^40");
    const long long bytes = 3ll * im.H * im.W;
    for (int j = 0; j < im.n_src; ++j) {
      if (im.op[j] < 0 || im.op[j] > 7) SRGD_EXT_FAIL(name + ": op outside 0 .. 7");
      if (const char* p = offset_problem(im.src_off[j])) SRGD_EXT_FAIL(name + ": " + p);
      s.add(im.src_off[j], bytes);
    }
    d.add(im.dst_off, bytes);
  }
  if (s.meets(src, d, dst)) SRGD_EXT_FAIL(name + ": the source images and the destination images overlap");
  for (int first = 0; first < n_images; first += SE_MAX_IMAGES) {     // one launch per SE_MAX_IMAGES images
    const int cnt = std::min(SE_MAX_IMAGES, n_images - first);
    SeTable<SE_MAX_SOURCES> tab;
    unsigned blocks = 0;
    for (int k = 0; k < SE_MAX_IMAGES; ++k) {
      tab.im[k] = SeImage<SE_MAX_SOURCES>{0u, 1, 1, 1, se_magic(1), 0u, 0ull, {}};
      for (int j = 0; j < SE_MAX_SOURCES; ++j) tab.im[k].s[j] = SeSource{0u, 0u};
    }
    for (int k = 0; k < cnt; ++k) {
      const srgd_selfens_image& im = images[first + k];
      SeImage<SE_MAX_SOURCES>& out = tab.im[k];
      out.dst16 = (unsigned)(im.dst_off >> 4);
      out.H = im.H;
      out.W = im.W;
      out.n = im.n_src;
      out.magic = se_magic(im.n_src);
      out.m01 = mean01 ? (unsigned long long)im.mean01_off : 0ull;
      for (int j = 0; j < im.n_src; ++j) out.s[j] = SeSource{(unsigned)(im.src_off[j] >> 4), (unsigned)im.op[j]};
      blocks = std::max(blocks, tiles_of(im.H, im.W));
    }
    hipLaunchKernelGGL(selfens_merge_kernel, dim3(blocks, (unsigned)cnt), dim3(SE_THREADS), 0, st, tab, (const unsigned char*)src,
                       (unsigned char*)dst, mean01);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_selfens_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_selfens_transform(const void* src, void* dst, const srgd_selfens_record* records_host, int n, void* stream) {
  return transform(src, dst, records_host, n, (hipStream_t)stream);
}

SRGD_EXT_EXPORT int srgd_selfens_merge(const void* src, void* dst_u8, float* mean01, const srgd_selfens_image* images_host, int n_images,
                                       void* stream) {
  return merge(src, dst_u8, mean01, images_host, n_images, (hipStream_t)stream);
}

}  // extern "C"
