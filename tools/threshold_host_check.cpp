// Stand-alone check of the host side of libsrgd_threshold (include/srgd_threshold.h) for a sanitizer build on the CPU: the quantile
// positions of n = 1..300, 2^24 + 1 and 2^31 - 1 against the definition, the scratch size, and every refusal of the device call
// (decided before anything is launched; the pointers are never dereferenced).  No GPU is used.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         srgd_amd/csrc/threshold.hip tools/threshold_host_check.cpp -o threshold_host_check && ./threshold_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/srgd_threshold.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static void positions(int64_t n) {
  const float qs[5] = {0.5f, 0.9f, 0.995f, 1.0f, 1e-7f};
  for (float q : qs) {
    int64_t lo = -1, hi = -1;
    float frac = -1.0f;
    EXPECT(srgd_threshold_position(n, q, &lo, &hi, &frac) == 0);
    const double pos = (double)q * (double)(n - 1);
    const int64_t want_lo = (int64_t)std::floor(pos);
    EXPECT(lo == want_lo && hi == (want_lo + 1 < n ? want_lo + 1 : n - 1) && frac == (float)(pos - (double)want_lo));
    EXPECT(lo >= 0 && lo <= hi && hi <= n - 1);
  }
}

static srgd_threshold_image image() {
  srgd_threshold_image m;
  std::memset(&m, 0, sizeof m);
  m.Hp = m.Wp = 256;
  m.top = m.left = 118;
  m.H = m.W = 20;
  m.box_t = 100;
  m.box_l = 110;
  m.box_h = 60;
  m.box_w = 40;
  return m;
}

static bool refused(const srgd_threshold_image* im, int n, float q, float w, uintptr_t img, uintptr_t xs, uintptr_t out, uintptr_t scr,
                    const char* word) {
  const int rc = srgd_threshold_step((float*)img, (float*)xs, im, n, q, w, (float*)out, (void*)scr, nullptr);
  return rc == -1 && std::strstr(srgd_threshold_last_error(), word) != nullptr;
}

int main() {
  for (int64_t n = 1; n <= 300; ++n) positions(n);
  positions((1ll << 24) + 1);
  positions((1ll << 31) - 1);
  int64_t lo, hi;
  float frac;
  EXPECT(srgd_threshold_position(0, 0.5f, &lo, &hi, &frac) == -1);
  EXPECT(srgd_threshold_position(5, 0.0f, &lo, &hi, &frac) == -1);
  EXPECT(srgd_threshold_position(5, 1.5f, &lo, &hi, &frac) == -1);
  EXPECT(srgd_threshold_position(5, std::numeric_limits<float>::quiet_NaN(), &lo, &hi, &frac) == -1);
  EXPECT(srgd_threshold_position(5, 0.5f, nullptr, &hi, &frac) == -1);
  EXPECT(srgd_threshold_scratch_bytes(0) == 0 && srgd_threshold_scratch_bytes(1) == 8448 && srgd_threshold_scratch_bytes(130) == 130ull * 8448);
  EXPECT(srgd_threshold_chunk_elems() == 4096);

  const uintptr_t img = 1u << 24, xs = 2u << 24, out = 3u << 24, scr = 4u << 24;       // never dereferenced: every call is refused
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  std::vector<srgd_threshold_image> one(1, image());
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, 0, xs, out, scr, "null"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img, 0, out, scr, "null"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img, xs, 0, scr, "null"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img, xs, out, 0, "null"));
  EXPECT(refused(nullptr, 1, 0.9f, 0.5f, img, xs, out, scr, "null"));
  EXPECT(refused(one.data(), 0, 0.9f, 0.5f, img, xs, out, scr, "n_images"));
  EXPECT(refused(one.data(), 1, 0.0f, 0.5f, img, xs, out, scr, "q must be"));
  EXPECT(refused(one.data(), 1, nan, 0.5f, img, xs, out, scr, "q must be"));
  EXPECT(refused(one.data(), 1, 1.5f, 0.5f, img, xs, out, scr, "q must be"));
  EXPECT(refused(one.data(), 1, 0.9f, nan, img, xs, out, scr, "finite"));
  EXPECT(refused(one.data(), 1, 0.9f, inf, img, xs, out, scr, "finite"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img + 2, xs, out, scr, "4-byte aligned"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img, xs, out, scr + 64, "256-byte aligned"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img, img + 8, out, scr, "overlapping buffers"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img, xs, out, xs + 256, "overlapping buffers"));
  EXPECT(refused(one.data(), 1, 0.9f, 0.5f, img, xs, scr + 1024, scr, "overlapping buffers"));
  struct Edit { int field, value; const char* word; };
  const Edit edits[] = {{0, 0, "bad size"}, {1, -1, "bad size"}, {2, 0, "bad canvas"}, {3, 149, "update box"}, {4, 157, "update box"},
                        {5, -1, "update box"}, {6, 99, "statistics box"}, {7, 109, "statistics box"}, {0, 43, "statistics box"},
                        {1, 33, "statistics box"}, {8, 26755, "bad canvas"}};
  for (const Edit& e : edits) {
    std::vector<srgd_threshold_image> bad(2, image());
    bad[1].canvas_off = 3 * 65536;
    srgd_threshold_image& m = bad[1];                    // the second image: every image is checked before the first launch
    int32_t* fields[] = {&m.H, &m.W, &m.Hp, &m.Wp, &m.box_h, &m.box_l, &m.top, &m.left};
    if (e.field == 8) m.Hp = m.Wp = e.value; else *fields[e.field] = e.value;
    EXPECT(refused(bad.data(), 2, 0.9f, 0.5f, img, xs, out, scr, e.word));
  }
  std::vector<srgd_threshold_image> two(2, image());
  EXPECT(refused(two.data(), 2, 0.9f, 0.5f, img, xs, out, scr, "overlapping canvases"));
  two[1].canvas_off = -1;
  EXPECT(refused(two.data(), 2, 0.9f, 0.5f, img, xs, out, scr, "offset outside"));
  std::printf(failures ? "threshold_host_check: %d FAILED\n" : "threshold_host_check: ok (%d failures)\n", failures);
  return failures ? 1 : 0;
}
