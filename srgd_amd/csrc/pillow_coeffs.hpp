// Pillow's resampling tables (src/libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc), restated once for every file
// that claims bit-exactness with Image.resize: per output a window of the input clipped to the image, double-precision weights
// renormalised to sum 1, converted to 22-bit fixed point (round half away from zero).  Host-only plain C++.  The arithmetic is in
// Pillow's order and in separate multiplications and additions (contraction is switched off inside every function, whatever the
// flags of the including file).  Limits and error texts belong to the callers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace srgd {

constexpr int PILLOW_PREC_BITS = 32 - 8 - 2;         // Pillow's PRECISION_BITS: 22

namespace pillow {

enum Filter { LANCZOS = 1, BILINEAR = 2, BICUBIC = 3 };             // Pillow's own numbers (Image.Resampling)
constexpr int MAX_TAPS = 64;                         // the widest window a row builder's buffer holds; every caller's limit lies below

inline double bicubic_weight(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

inline double bilinear_weight(double x) {
#pragma clang fp contract(off)
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

inline double sinc_weight(double x) {
#pragma clang fp contract(off)
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

inline double lanczos_weight(double x) {
#pragma clang fp contract(off)
  if (-3.0 <= x && x < 3.0) return sinc_weight(x) * sinc_weight(x / 3);
  return 0.0;
}

// 0.0: not a filter of this header
inline double filter_support(int filter) { return filter == BICUBIC ? 2.0 : (filter == BILINEAR ? 1.0 : (filter == LANCZOS ? 3.0 : 0.0)); }

// Pillow's ksize of an axis: the stride of its coefficient rows
inline int ksize(int in_size, int out_size, int filter) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

// Output xx of out_size from in_size: the first input index, the number of taps and the fixed-point coefficients from that index
// on, in k[0 .. cap) (zero beyond the last tap).  cap >= ksize(in_size, out_size, filter) holds every window; cap <= MAX_TAPS.
inline void row(int in_size, int out_size, int filter, int xx, int* first, int* count, int32_t* k, int cap) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(filter) * filterscale, ss = 1.0 / filterscale;
  const double center = (xx + 0.5) * scale;
  double w[MAX_TAPS], ww = 0.0;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (cap > MAX_TAPS) cap = MAX_TAPS;
  if (xmax > cap) xmax = cap;                                          // never taken: ksize bounds every window
  for (int x = 0; x < xmax; ++x) {
    const double arg = (x + xmin - center + 0.5) * ss;
    w[x] = filter == BICUBIC ? bicubic_weight(arg) : (filter == BILINEAR ? bilinear_weight(arg) : lanczos_weight(arg));
    ww += w[x];
  }
  for (int x = 0; x < cap; ++x) k[x] = 0;
  for (int x = 0; x < xmax; ++x) {
    if (ww != 0.0) w[x] /= ww;
    k[x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << PILLOW_PREC_BITS)) : (int)(0.5 + w[x] * (1 << PILLOW_PREC_BITS));
  }
  *first = xmin;
  *count = xmax;
}

// The table of an axis: bounds [out_size][2] = (first input index, count), coeffs [out_size][ksize]
inline void axis_table(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coeffs) {
  const int ks = ksize(in_size, out_size, filter);
  for (int xx = 0; xx < out_size; ++xx) row(in_size, out_size, filter, xx, bounds + 2 * xx, bounds + 2 * xx + 1, coeffs + (size_t)xx * (size_t)ks, ks);
}

// The bicubic x4 vectors, which do not depend on the size n >= 5: they are taken from 256 <-> 64.
//   reduction 4n -> n:    five vectors of 16 taps: rows 0, 1, the interior (10), n-2, n-1;
//   enlargement n -> 4n:  sixteen vectors of 4 taps: outputs 0 .. 5, the phases 0 .. 3 (outputs 6 .. 9), outputs 4n-6 .. 4n-1.
// `framed`: laid on the frame of their output - [4i - 6, 4i + 10) for the reduction, [floor((j - 6) / 4), + 4) for the
// enlargement - with zeros on the taps in front of the image; otherwise from the window's first input on.
constexpr int X4_REF_N = 64;
constexpr int X4_REDUCE_TAPS = 16, X4_ENLARGE_TAPS = 4;

inline void x4_vector(int in_size, int out_size, int xx, int frame, bool framed, int32_t* out, int taps) {
  int first, count;
  int32_t k[X4_REDUCE_TAPS];
  row(in_size, out_size, BICUBIC, xx, &first, &count, k, X4_REDUCE_TAPS);
  const int shift = framed ? first - frame : 0;
  for (int t = 0; t < taps; ++t) out[t] = (t >= shift && t - shift < count) ? k[t - shift] : 0;
}

inline void x4_reduce_vectors(int32_t out[5][X4_REDUCE_TAPS], bool framed) {
  const int rows[5] = {0, 1, 10, X4_REF_N - 2, X4_REF_N - 1};
  for (int v = 0; v < 5; ++v)                                          // shift on the frame: 6, 2, 0, 0, 0
    x4_vector(4 * X4_REF_N, X4_REF_N, rows[v], 4 * rows[v] - 6, framed, out[v], X4_REDUCE_TAPS);
}

inline void x4_enlarge_vectors(int32_t out[16][X4_ENLARGE_TAPS], bool framed) {
  for (int v = 0; v < 16; ++v) {                                       // shift on the frame: 2, 2, 1, 1, 1, 1, then zeros
    const int j = v < 10 ? v : 4 * X4_REF_N - 16 + v;
    x4_vector(X4_REF_N, 4 * X4_REF_N, j, (j + 2) / 4 - 2, framed, out[v], X4_ENLARGE_TAPS);
  }
}

}  // namespace pillow
}  // namespace srgd
