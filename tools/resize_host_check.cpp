// Stand-alone check of the host side of libsrgd_resize (include/srgd_resize.h) for a sanitizer build on the CPU: the tables of every
// axis pair 1..40 x 1..40 within the ratio limit, of the test cases' pairs and of the largest geometry, all three filters, into
// buffers of exactly the documented size, and every refusal of the device call (decided before anything is launched; the pointers
// are never dereferenced).  No GPU is used.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         srgd_amd/csrc/resize.hip tools/resize_host_check.cpp -o resize_host_check && ./resize_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/srgd_resize.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static long long table(int in_size, int out_size, int filter) {
  const int ksize = srgd_resize_ksize(in_size, out_size, filter);
  EXPECT(ksize >= 3 && ksize <= SRGD_RESIZE_MAX_TAPS && (ksize & 1) == 1);
  std::vector<int32_t> bounds(2 * (size_t)out_size), coeffs((size_t)out_size * (size_t)ksize);
  EXPECT(srgd_resize_coeffs(in_size, out_size, filter, bounds.data(), coeffs.data()) == 0);
  long long sum = 0;
  for (int xx = 0; xx < out_size; ++xx) {
    const int xmin = bounds[2 * xx], count = bounds[2 * xx + 1];
    EXPECT(xmin >= 0 && count >= 1 && count <= ksize && xmin + count <= in_size);
    long long row = 0;
    for (int x = 0; x < ksize; ++x) {
      row += coeffs[(size_t)xx * ksize + x];
      EXPECT(x < count || coeffs[(size_t)xx * ksize + x] == 0);
    }
    EXPECT(row > (1 << 22) - 64 && row < (1 << 22) + 64);                // a renormalised window sums to one, up to the roundings
    sum += row;
  }
  return sum;
}

int main() {
  const int filters[3] = {SRGD_RESIZE_LANCZOS, SRGD_RESIZE_BILINEAR, SRGD_RESIZE_BICUBIC};
  const int cases[][2] = {{200, 25}, {48, 6}, {64, 8}, {6, 48}, {8, 64}, {129, 43}, {67, 100}, {65, 31}, {52, 26}, {52, 39}, {100, 85},
                          {100, 86}, {64, 88}, {16384, 2048}, {2048, 16384}, {16384, 16383}, {1, 8}, {8, 1}};
  long long tables = 0, sum = 0;
  for (const int filter : filters) {
    for (int a = 1; a <= 40; ++a) {
      for (int b = 1; b <= 40; ++b) {
        if (a <= SRGD_RESIZE_MAX_RATIO * b && b <= SRGD_RESIZE_MAX_RATIO * a) sum += table(a, b, filter), ++tables;
      }
    }
    for (const auto& c : cases) sum += table(c[0], c[1], filter), ++tables;
  }
  // the host functions' refusals
  int32_t word = 0;
  EXPECT(srgd_resize_ksize(16, 1, SRGD_RESIZE_LANCZOS) == -1 && std::strstr(srgd_resize_last_error(), "ratio"));
  EXPECT(srgd_resize_ksize(0, 1, SRGD_RESIZE_BICUBIC) == -1 && std::strstr(srgd_resize_last_error(), "bad size"));
  EXPECT(srgd_resize_ksize(8, 8, 7) == -1 && std::strstr(srgd_resize_last_error(), "unknown filter"));
  EXPECT(srgd_resize_coeffs(8, 8, SRGD_RESIZE_BICUBIC, nullptr, &word) == -1 && std::strstr(srgd_resize_last_error(), "null"));
  EXPECT(srgd_resize_coeffs(17, 2, SRGD_RESIZE_BICUBIC, &word, &word) == -1 && word == 0);
  // the device call's refusals: nothing is launched, no pointer is dereferenced
  void* const src = (void*)(uintptr_t)(1ull << 30);
  void* const dst = (void*)(uintptr_t)(2ull << 30);
  void* const tab = (void*)(uintptr_t)(3ull << 30);
  void* const scr = (void*)(uintptr_t)(4ull << 30);
  const int64_t big = 1ll << 40;
  const srgd_resize_image good = {0, 0, 0, 40, 52, 20, 26};
  int refusals = 0;
  auto refused = [&](const void* s, void* d, const srgd_resize_image* im, int n, int filter, const void* t, int64_t tb, void* sc, int64_t sb,
                     const char* phrase) {
    const int rc = srgd_resize_u8_images(s, d, im, n, filter, t, tb, sc, sb, nullptr);
    EXPECT(rc == -1 && std::strstr(srgd_resize_last_error(), phrase) != nullptr);
    ++refusals;
  };
  refused(nullptr, dst, &good, 1, 3, tab, big, scr, big, "null");
  refused(src, nullptr, &good, 1, 3, tab, big, scr, big, "null");
  refused(src, dst, nullptr, 1, 3, tab, big, scr, big, "null");
  refused(src, dst, &good, 1, 3, nullptr, big, scr, big, "null");
  refused(src, dst, &good, 1, 3, tab, big, nullptr, big, "null");
  refused(src, dst, &good, 0, 3, tab, big, scr, big, "n_images");
  refused(src, dst, &good, 1, 0, tab, big, scr, big, "unknown filter");
  refused(src, dst, &good, 1, 3, (char*)tab + 4, big, scr, big, "tables must be");
  refused(src, dst, &good, 1, 3, tab, big, (char*)scr + 8, big, "scratch must be");
  refused(src, dst, &good, 1, 3, tab, 100, scr, big, "tables_bytes");
  refused(src, dst, &good, 1, 3, tab, big, scr, 3 * 40 * 26 - 1, "scratch_bytes");
  refused(src, src, &good, 1, 3, tab, big, scr, big, "overlap");
  srgd_resize_image group[3] = {good, good, good};
  group[1].src_off = 16 * 1000, group[1].dst_off = 16 * 500, group[2].src_off = 16 * 2000, group[2].dst_off = 16 * 1000;
  const srgd_resize_image bad[] = {{0, 0, 0, 0, 52, 20, 26},       {0, 0, 0, 40, 52, 20, 16385}, {0, 0, 0, 161, 52, 20, 26}, {0, 0, 0, 16, 16, 1, 1},
                                   {8, 0, 0, 40, 52, 20, 26},      {0, 24, 0, 40, 52, 20, 26},   {0, 0, 4, 40, 52, 20, 26},  {-16, 0, 0, 40, 52, 20, 26},
                                   {0, 1ll << 36, 0, 40, 52, 20, 26}};
  const char* phrases[] = {"bad size", "bad size", "ratio", "ratio", "multiple of 16", "multiple of 16", "multiple of 16", "outside", "outside"};
  for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
    for (int at = 0; at < 3; ++at) {                                      // one bad image anywhere in a group stops the call
      srgd_resize_image g[3] = {group[0], group[1], group[2]};
      g[at] = bad[i];
      refused(src, dst, g, 3, 3, tab, big, scr, big, phrases[i]);
    }
  }
  std::printf("%lld tables (coefficient sum %lld), %d refusals, %d failures\n", tables, sum, refusals, failures);
  return failures == 0 ? 0 : 1;
}
