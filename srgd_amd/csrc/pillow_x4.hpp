// The selectors of Pillow's fixed x4 bicubic vectors and the byte extractor of the 8-bit x4 kernels, once (consistency.hip,
// backproject.hip, guidance.hip).  A header, not a library: each file includes it into its one translation unit, so the libraries
// still share no symbol.
//
// The window facts.  Reduction (4n -> n, n >= 5): output i in 2 .. n-3 reads the 16 inputs from 4i - 6 with one symmetric vector;
// outputs 0, 1, n-2, n-1 read 10, 14, 14, 10 inputs of the clipped window with vectors of their own.  Enlargement (n -> 4n): output j
// in 6 .. 4n-7 reads the 4 inputs from (j - 6) / 4 with the vector of its phase (j - 6) % 4; outputs 0 .. 5 and 4n-6 .. 4n-1 have
// vectors of their own.  No vector depends on n (pillow_coeffs.hpp: x4_reduce_vectors, x4_enlarge_vectors hold them in this order).
#pragma once

#include <hip/hip_runtime.h>

#include "ext_common.hpp"

namespace srgd {
namespace {

// the reduction's vector of output index i of n
__device__ __forceinline__ int x4_down_vector(int i, int n) { return i == 0 ? 0 : (i == 1 ? 1 : (i == n - 2 ? 3 : (i == n - 1 ? 4 : 2))); }
// the enlargement's vector of output index j of n4 = 4n (any vector for an index beyond the image: its result is never used)
__device__ __forceinline__ int x4_up_vector(int j, int n4) { return j < 6 ? j : (j >= n4 - 6 ? min(15, 10 + j - (n4 - 6)) : 6 + ((j + 2) & 3)); }
// byte k of a run of dwords
__device__ __forceinline__ int u8_of(const unsigned* d, int k) { return (int)((d[k >> 2] >> (8 * (k & 3))) & 0xffu); }

}  // namespace
}  // namespace srgd
