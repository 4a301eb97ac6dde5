// Dynamic thresholding of the tiled DDPM sampler's prediction of the clean image on the GPU (engine extension, absent upstream;
// Imagen's percentile clipping): per image, s = max(1, the q-quantile of |x_start| inside the crop box), x_start is clipped to
// [-s, s] and divided by s inside the box the step wrote, and img receives weight_img times the change.  The definition - keys,
// position, threshold, apply - is fixed in include/srgd_threshold.h and restated here in short.
//
// The quantile is an exact order statistic: a radix select on key(v) = bits(v) & 0x7fffffff (31 bits: digits of 11, 10 and 10 bits,
// most significant first).  Two states (prefix, remaining rank) per image - one for rank lo, one for rank hi = lo + 1 - walk down the
// digits together; they share their prefix until the two ranks fall into different counters of a pass, and from then on a pass counts
// under both prefixes (the two halves of the 2048 counters).
//
// Work split.  blockIdx.y is the image (its record travels in the kernel argument).
//   hist:  one workgroup of 256 threads per 4096 keys of the statistics box (3 planes, row-major inside the box).  Counters in LDS;
//          a wave first folds the lanes that share a counter - up to 4 rounds of (first open lane's counter, ballot of the lanes on it,
//          one LDS add of the count) - because |x_start| concentrates in a few exponent bins and per-lane LDS atomics on one address
//          serialise; the lanes left over (spread digits) add 1 each.  The workgroup then adds its non-empty counters to the image's
//          2048 counters in the scratch, one unsigned integer atomic each.
//   scan:  one workgroup per image: reads the counters (and clears them for the next pass), finds for either state the counter its
//          rank falls into - per-thread sums of 8 or 4 consecutive counters, an inclusive scan over the 256 threads, a walk by the
//          one thread whose range holds the rank - and writes (prefix << bits | counter, rank - count below).  After the third pass the
//          prefixes are the keys a_lo and a_hi; the scan forms s and writes it to the state and to s_out.
//   apply: one workgroup per 2048 elements of a plane of the update box (blockIdx.z: the plane); a thread reads x_start at an
//          element, writes it, and reads and writes img there only where the value changed - dword accesses along the row.
// Integer sums are order-independent: every image comes out bit-identical alone, in any group, at any offset.  LDS: hist 8,192 bytes,
// scan 8,192 + 1,024 + 16.  Bytes moved per call and element: 3 x 4 read in the statistics box, 4 + 4 (x_start) and up to 4 + 4
// (img) in the update box.
// Compiled with -ffp-contract=off: the threshold and the update are separate multiplications and additions.
#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/srgd_threshold.h"
#include "ext_common.hpp"

// This file is a library of its own (libsrgd_threshold.so, include/srgd_threshold.h): it shares no symbol with the engine or the other nine
// extension libraries; ext_common.hpp is their common host plumbing (pillow_resample.hpp and pillow_x4.hpp, the code some of them have in
// common, are headers too: no symbol is shared).
namespace srgd {
namespace {

constexpr int TH_THREADS = 256;
constexpr int TH_PER_THREAD = 16;
constexpr int TH_CHUNK = TH_THREADS * TH_PER_THREAD;     // keys of one workgroup of the histogram kernel: 4096
constexpr int TH_BINS = 2048;                            // counters per image: pass 0 all of them, passes 1 and 2 two halves
constexpr int TH_HALF = TH_BINS / 2;
constexpr int TH_STATE = TH_BINS;                        // words of an image's scratch: counters, then the state
constexpr int TH_WORDS = TH_BINS + 64;                   // 8448 bytes per image, a multiple of 256
constexpr int TH_S_WORD = TH_STATE + 4;                  // state: prefix lo, prefix hi, rank lo, rank hi, s
constexpr int TH_APPLY_PER_THREAD = 8;
constexpr int TH_APPLY_CHUNK = TH_THREADS * TH_APPLY_PER_THREAD;
constexpr int TH_MAX_IMAGES = 128;                       // records travel as kernel arguments (3 KiB and 2 KiB)
constexpr int TH_FOLD_ROUNDS = 4;
static_assert(TH_WORDS * 4 % 256 == 0, "every image's part of the scratch is 256-byte aligned");
static_assert(TH_BINS % TH_THREADS == 0 && TH_HALF % TH_THREADS == 0, "the scan gives every thread the same number of counters");

struct ThBox {
  long long base;                                        // element of the box's first pixel in plane 0 of img and x_start
  int plane, Wp;                                         // Hp * Wp; the canvas row
  int h, w;                                              // the box
};
struct ThBoxes { ThBox im[TH_MAX_IMAGES]; };
struct ThRank { unsigned lo, hi; float frac; unsigned pad; };
struct ThRanks { ThRank im[TH_MAX_IMAGES]; };

__host__ __device__ inline int th_shift(int pass) { return pass == 0 ? 20 : (pass == 1 ? 10 : 0); }

// One pass of the select: counts digit `pass` of the keys of the statistics box that lie under the prefix of either state.
__global__ __launch_bounds__(TH_THREADS) void threshold_hist_kernel(ThBoxes tab, const float* __restrict__ x_start,
                                                                    unsigned* __restrict__ scratch, int first, int pass) {
  __shared__ unsigned hist[TH_BINS];
  const ThBox im = tab.im[blockIdx.y];
  const unsigned hw = (unsigned)im.h * (unsigned)im.w, n = 3u * hw;       // n < 2^31
  const unsigned e0 = blockIdx.x * (unsigned)TH_CHUNK;
  if (e0 >= n) return;                                                    // the grid is as wide as the launch's largest image
  const int tid = (int)threadIdx.x, lane = tid & 63;
  unsigned* mine = scratch + (size_t)(first + (int)blockIdx.y) * TH_WORDS;
  for (int i = tid; i < TH_BINS; i += TH_THREADS) hist[i] = 0u;
  unsigned plo = 0u, phi = 0u;
  if (pass > 0) {
    plo = mine[TH_STATE];
    phi = mine[TH_STATE + 1];
  }
  __syncthreads();
  const int shift = th_shift(pass);
  const unsigned mask = pass == 0 ? (unsigned)TH_BINS - 1u : (unsigned)TH_HALF - 1u;
  const float* src = x_start + im.base;
#pragma unroll 4
  for (int k = 0; k < TH_PER_THREAD; ++k) {
    const unsigned e = e0 + (unsigned)(k * TH_THREADS + tid);
    bool open = e < n;
    unsigned bin = 0u;
    if (open) {
      const unsigned c = e / hw, r = e - c * hw;
      const unsigned y = r / (unsigned)im.w, x = r - y * (unsigned)im.w;
      const unsigned key = __float_as_uint(src[(int)c * im.plane + (int)y * im.Wp + (int)x]) & 0x7fffffffu;   // < 3 * Hp * Wp < 2^31
      bin = (key >> shift) & mask;
      if (pass > 0) {
        const unsigned upper = key >> (shift + 10);
        if (upper == plo) {
        } else if (upper == phi) {
          bin += (unsigned)TH_HALF;
        } else {
          open = false;
        }
      }
    }
    // fold the lanes of the wave that share a counter (wave-uniform loop)
    unsigned long long rest = __ballot(open);
    for (int round = 0; round < TH_FOLD_ROUNDS && rest != 0ull; ++round) {
      const int leader = __ffsll((long long)rest) - 1;
      const unsigned lead_bin = (unsigned)__shfl((int)bin, leader, 64);
      const bool same = open && bin == lead_bin;
      const unsigned long long m = __ballot(same);
      if (lane == leader) atomicAdd(&hist[lead_bin], (unsigned)__popcll(m));
      if (same) open = false;
      rest &= ~m;
    }
    if (open) atomicAdd(&hist[bin], 1u);
  }
  __syncthreads();
  for (int i = tid; i < TH_BINS; i += TH_THREADS) {
    const unsigned cnt = hist[i];
    if (cnt != 0u) atomicAdd(&mine[i], cnt);                              // integer: the sum does not depend on the order
  }
}

// Advances the two states of every image by one digit; after the last pass forms s.
__global__ __launch_bounds__(TH_THREADS) void threshold_scan_kernel(ThRanks tab, unsigned* __restrict__ scratch, float* __restrict__ s_out,
                                                                    int first, int pass) {
  __shared__ unsigned hist[TH_BINS];
  __shared__ unsigned part[TH_THREADS];
  __shared__ unsigned found[4];                                           // prefix lo, prefix hi, rank lo, rank hi
  const int tid = (int)threadIdx.x;
  unsigned* mine = scratch + (size_t)(first + (int)blockIdx.y) * TH_WORDS;
  for (int i = tid; i < TH_BINS; i += TH_THREADS) {
    hist[i] = mine[i];
    mine[i] = 0u;                                                         // the next pass counts from zero
  }
  const ThRank rk = tab.im[blockIdx.y];
  unsigned prefix[2] = {0u, 0u}, rank[2] = {rk.lo, rk.hi};
  if (pass > 0) {
    prefix[0] = mine[TH_STATE];
    prefix[1] = mine[TH_STATE + 1];
    rank[0] = mine[TH_STATE + 2];
    rank[1] = mine[TH_STATE + 3];
  }
  const int bits = pass == 0 ? 11 : 10;
  const int nbins = pass == 0 ? TH_BINS : TH_HALF;
  const int per = nbins / TH_THREADS;
  if (tid < 4) found[tid] = tid < 2 ? prefix[tid] << bits : 0u;
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int base = (s == 1 && pass > 0 && prefix[1] != prefix[0]) ? TH_HALF : 0;
    unsigned sum = 0u;
    for (int j = 0; j < per; ++j) sum += hist[base + tid * per + j];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < TH_THREADS; d <<= 1) {                            // inclusive scan over the threads
      const unsigned add = tid >= d ? part[tid - d] : 0u;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    const unsigned incl = part[tid], excl = incl - sum;
    if (rank[s] >= excl && rank[s] < incl) {                              // one thread: the counts below the rank end inside its range
      unsigned acc = excl;
      for (int j = 0; j < per; ++j) {
        const unsigned cnt = hist[base + tid * per + j];
        if (rank[s] < acc + cnt) {
          found[s] = (prefix[s] << bits) | (unsigned)(tid * per + j);
          found[2 + s] = rank[s] - acc;
          break;
        }
        acc += cnt;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    mine[TH_STATE] = found[0];
    mine[TH_STATE + 1] = found[1];
    mine[TH_STATE + 2] = found[2];
    mine[TH_STATE + 3] = found[3];
    if (pass == 2) {                                                      // the prefixes are the keys a_lo and a_hi
      const float a_lo = __uint_as_float(found[0]), a_hi = __uint_as_float(found[1]);
      const float diff = a_hi - a_lo;
      const float prod = rk.frac * diff;
      const float s_raw = a_lo + prod;
      const float s = (s_raw < 1.0f) ? 1.0f : s_raw;                      // a NaN stays
      mine[TH_S_WORD] = __float_as_uint(s);
      s_out[first + (int)blockIdx.y] = s;
    }
  }
}

// x_start = clip(x_start, -s, s) / s and img += weight_img * (the change) inside the update box.
__global__ __launch_bounds__(TH_THREADS) void threshold_apply_kernel(ThBoxes tab, float* __restrict__ img, float* __restrict__ x_start,
                                                                     const unsigned* __restrict__ scratch, float weight_img, int first) {
  const ThBox im = tab.im[blockIdx.y];
  const unsigned n = (unsigned)im.h * (unsigned)im.w;                     // < 2^31 / 3
  const unsigned e0 = blockIdx.x * (unsigned)TH_APPLY_CHUNK;
  if (e0 >= n) return;
  const float s = __uint_as_float(scratch[(size_t)(first + (int)blockIdx.y) * TH_WORDS + TH_S_WORD]);
  const long long canvas = im.base + (long long)blockIdx.z * im.plane;
#pragma unroll
  for (int k = 0; k < TH_APPLY_PER_THREAD; ++k) {
    const unsigned e = e0 + (unsigned)(k * TH_THREADS) + threadIdx.x;
    if (e >= n) break;
    const unsigned y_ = e / (unsigned)im.w, x_ = e - y_ * (unsigned)im.w;
    const long long o = canvas + (int)y_ * im.Wp + (int)x_;
    const float v = x_start[o];
    const float t = v < -s ? -s : (v > s ? s : v);
    const float y = t / s;
    const float d = y - v;
    x_start[o] = y;
    if (d != 0.0f) {
      const float prod = weight_img * d;
      img[o] = img[o] + prod;
    }
  }
}

int position(int64_t n, float q, int64_t* lo, int64_t* hi, float* frac) {
  const std::string name("srgd_threshold_position");
  if (!lo || !hi || !frac) SRGD_EXT_FAIL(name + ": null argument");
  if (n < 1) SRGD_EXT_FAIL(name + ": n must be >= 1");
  if (!(q > 0.0f && q <= 1.0f)) SRGD_EXT_FAIL(name + ": q must be in (0, 1]");
  const double pos = (double)q * (double)(n - 1);
  const double fl = std::floor(pos);
  *lo = (int64_t)fl;
  *hi = std::min<int64_t>(*lo + 1, n - 1);
  *frac = (float)(pos - fl);
  return 0;
}

int threshold_step(float* img, float* x_start, const srgd_threshold_image* images, int n_images, float q, float weight_img,
                   float* s_out, void* scratch, hipStream_t st) {
  const std::string name("srgd_threshold_step");
  if (n_images < 1) SRGD_EXT_FAIL(name + ": n_images must be >= 1");
  if (!img || !x_start || !images || !s_out || !scratch) SRGD_EXT_FAIL(name + ": null argument");
  if (!(q > 0.0f && q <= 1.0f)) SRGD_EXT_FAIL(name + ": q must be in (0, 1]");
  if (!std::isfinite(weight_img)) SRGD_EXT_FAIL(name + ": weight_img must be finite");
  if ((((uintptr_t)img | (uintptr_t)x_start | (uintptr_t)s_out) & 3u) != 0) SRGD_EXT_FAIL(name + ": img, x_start and s_out must be 4-byte aligned");
  if (((uintptr_t)scratch & 255u) != 0) SRGD_EXT_FAIL(name + ": scratch must be 256-byte aligned");
  long long lo = 0, hi = 0;                              // the elements the call covers in img / x_start
  for (int i = 0; i < n_images; ++i) {                   // every image is checked before the first launch
    const srgd_threshold_image& m = images[i];
    if (m.H < 1 || m.W < 1) SRGD_EXT_FAIL(name + ": bad size (H and W must be >= 1)");
    if (m.Hp < 1 || m.Wp < 1 || 3ll * m.Hp * m.Wp >= (1ll << 31)) SRGD_EXT_FAIL(name + ": bad canvas (3*Hp*Wp must be in 1 .. 2^31 - 1)");
    if (m.box_t < 0 || m.box_l < 0 || m.box_h < 1 || m.box_w < 1 || (long long)m.box_t + m.box_h > m.Hp || (long long)m.box_l + m.box_w > m.Wp)
      SRGD_EXT_FAIL(name + ": the update box leaves its canvas");
    if (m.top < m.box_t || m.left < m.box_l || (long long)m.top + m.H > (long long)m.box_t + m.box_h ||
        (long long)m.left + m.W > (long long)m.box_l + m.box_w)
      SRGD_EXT_FAIL(name + ": the statistics box leaves the update box");
    if (m.canvas_off < 0 || m.canvas_off >= (1ll << 40)) SRGD_EXT_FAIL(name + ": offset outside [0, 2^40)");
    const long long canvas = 3ll * m.Hp * m.Wp;
    lo = i == 0 ? m.canvas_off : std::min<long long>(lo, m.canvas_off);
    hi = i == 0 ? m.canvas_off + canvas : std::max<long long>(hi, m.canvas_off + canvas);
  }
  for (int i = 0; i < n_images; ++i)
    for (int j = i + 1; j < n_images; ++j) {
      const Range a{images[i].canvas_off, images[i].canvas_off + 3ll * images[i].Hp * images[i].Wp};
      const Range b{images[j].canvas_off, images[j].canvas_off + 3ll * images[j].Hp * images[j].Wp};
      if (a.meets(b)) SRGD_EXT_FAIL(name + ": overlapping canvases");
    }
  const long long scr_bytes = (long long)n_images * TH_WORDS * 4;
  const Range r_img{(long long)(intptr_t)img + 4 * lo, (long long)(intptr_t)img + 4 * hi};
  const Range r_xs{(long long)(intptr_t)x_start + 4 * lo, (long long)(intptr_t)x_start + 4 * hi};
  const Range r_s{(long long)(intptr_t)s_out, (long long)(intptr_t)s_out + 4ll * n_images};
  const Range r_scr{(long long)(intptr_t)scratch, (long long)(intptr_t)scratch + scr_bytes};
  if (r_img.meets(r_xs) || r_img.meets(r_s) || r_img.meets(r_scr) || r_xs.meets(r_s) || r_xs.meets(r_scr) || r_s.meets(r_scr))
    SRGD_EXT_FAIL(name + ": overlapping buffers (img, x_start, s_out and scratch are disjoint)");
  if (hipMemsetAsync(scratch, 0, (size_t)scr_bytes, st) != hipSuccess) {
    const hipError_t err = hipGetLastError();
    SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  for (int first = 0; first < n_images; first += TH_MAX_IMAGES) {     // one launch sequence per TH_MAX_IMAGES images
    const int cnt = std::min(TH_MAX_IMAGES, n_images - first);
    ThBoxes stats, update;
    ThRanks ranks;
    unsigned max_chunks = 0, max_apply = 0;
    for (int k = 0; k < TH_MAX_IMAGES; ++k) {
      stats.im[k] = update.im[k] = ThBox{0ll, 0, 0, 0, 0};
      ranks.im[k] = ThRank{0u, 0u, 0.0f, 0u};
    }
    for (int k = 0; k < cnt; ++k) {
      const srgd_threshold_image& m = images[first + k];
      const int plane = m.Hp * m.Wp;
      stats.im[k] = ThBox{m.canvas_off + (long long)m.top * m.Wp + m.left, plane, m.Wp, m.H, m.W};
      update.im[k] = ThBox{m.canvas_off + (long long)m.box_t * m.Wp + m.box_l, plane, m.Wp, m.box_h, m.box_w};
      const int64_t n = 3ll * m.H * m.W;
      int64_t p_lo = 0, p_hi = 0;
      float frac = 0.0f;
      position(n, q, &p_lo, &p_hi, &frac);
      ranks.im[k] = ThRank{(unsigned)p_lo, (unsigned)p_hi, frac, 0u};
      max_chunks = std::max(max_chunks, (unsigned)((n + TH_CHUNK - 1) / TH_CHUNK));
      max_apply = std::max(max_apply, (unsigned)(((long long)m.box_h * m.box_w + TH_APPLY_CHUNK - 1) / TH_APPLY_CHUNK));
    }
    for (int pass = 0; pass < 3; ++pass) {
      hipLaunchKernelGGL(threshold_hist_kernel, dim3(max_chunks, (unsigned)cnt), dim3(TH_THREADS), 0, st, stats, (const float*)x_start,
                         (unsigned*)scratch, first, pass);
      hipLaunchKernelGGL(threshold_scan_kernel, dim3(1u, (unsigned)cnt), dim3(TH_THREADS), 0, st, ranks, (unsigned*)scratch, s_out, first,
                         pass);
    }
    hipLaunchKernelGGL(threshold_apply_kernel, dim3(max_apply, (unsigned)cnt, 3u), dim3(TH_THREADS), 0, st, update, img, x_start,
                       (const unsigned*)scratch, weight_img, first);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) SRGD_EXT_FAIL(name + ": " + hipGetErrorString(err));
  }
  return 0;
}

}  // namespace
}  // namespace srgd

using namespace srgd;

extern "C" {

SRGD_EXT_EXPORT const char* srgd_threshold_last_error(void) { return g_err.c_str(); }

SRGD_EXT_EXPORT int srgd_threshold_position(int64_t n, float q, int64_t* lo, int64_t* hi, float* frac) { return position(n, q, lo, hi, frac); }

SRGD_EXT_EXPORT uint64_t srgd_threshold_scratch_bytes(int n_images) { return n_images < 1 ? 0ull : (uint64_t)n_images * TH_WORDS * 4ull; }

SRGD_EXT_EXPORT int srgd_threshold_chunk_elems(void) { return TH_CHUNK; }

SRGD_EXT_EXPORT int srgd_threshold_step(float* img, float* x_start, const srgd_threshold_image* images_host, int n_images, float q,
                                        float weight_img, float* s_out, void* scratch, void* stream) {
  return threshold_step(img, x_start, images_host, n_images, q, weight_img, s_out, scratch, (hipStream_t)stream);
}

}  // extern "C"
