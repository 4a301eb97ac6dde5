// Host plumbing shared by the extension libraries (metrics, ensemble, consistency, backproject, guidance, solver, resize, alpha,
// threshold, selfens): the last-error string behind every srgd_<name>_last_error, the export attribute, byte ranges for the
// overlap checks, and Pillow's 8-bit clip for the integer kernels.  Each of these libraries is ONE translation unit: the error
// string has internal linkage, so a library of several files would hold several.  The engine's own plumbing is common.hpp, which is
// deliberately not included here (its set_error is defined in engine.hip).  What some of the libraries have in common beyond this
// plumbing is headers as well, each included into the one translation unit of its users, so that no library shares a SYMBOL with
// another: pillow_resample.hpp, the general two-pass 8-bit resize (kernel bodies and host driver) of resize.hip and alpha.hip, and
// pillow_x4.hpp, the selectors of the x4 vectors and the byte extractor of consistency.hip, backproject.hip and guidance.hip.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>

#include <hip/hip_runtime.h>

#include "pillow_coeffs.hpp"                         // PILLOW_PREC_BITS

namespace srgd {
namespace {

thread_local std::string g_err;                      // what the library's last-error entry returns
#define SRGD_EXT_FAIL(msg)       \
  do {                           \
    g_err = std::string(msg);    \
    return -1;                   \
  } while (0)
#define SRGD_EXT_EXPORT __attribute__((visibility("default")))

// n rounded up to a multiple of a, a power of two
template <typename T>
__host__ __device__ constexpr T round_up(T n, T a) { return (n + (a - 1)) & ~(a - 1); }

// Bytes [lo, hi): of the address space, or of a buffer whose base address `meets` adds - there `add` grows the range over the
// images of a call.
struct Range {
  long long lo = 0, hi = 0;
  bool any = false;
  Range() = default;
  Range(long long lo_, long long hi_) : lo(lo_), hi(hi_), any(true) {}
  void add(long long off, long long bytes) {
    lo = any ? std::min(lo, off) : off;
    hi = any ? std::max(hi, off + bytes) : off + bytes;
    any = true;
  }
  bool meets(const Range& other) const { return lo < other.hi && other.lo < hi; }
  bool meets(const void* base, const Range& other, const void* other_base) const {
    const long long a = (long long)(intptr_t)base, b = (long long)(intptr_t)other_base;
    return Range(a + lo, a + hi).meets(Range(b + other.lo, b + other.hi));
  }
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> PILLOW_PREC_BITS;             // arithmetic shift, as Pillow's clip8 lookup index
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace
}  // namespace srgd
