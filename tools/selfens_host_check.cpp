// Stand-alone check of the host side of libsrgd_selfens (include/srgd_selfens.h) for a sanitizer build on the CPU: every refusal of
// srgd_selfens_transform and srgd_selfens_merge (decided before anything is launched; the pointers are never dereferenced) and the
// record validation at its limits - the largest sizes with 3*h*w < 2^31 on both sides of the bound, the offsets at both ends of
// [0, 2^36), n_src at 0, 1, 8 and 9, every op from -1 to 8.  A record that is valid is shown to be valid by making the call fail on
// something checked after the records (source and destination that overlap).  No GPU is used.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         srgd_amd/csrc/selfens.hip tools/selfens_host_check.cpp -o selfens_host_check && ./selfens_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/srgd_selfens.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static const uintptr_t SRC = (uintptr_t)1 << 40, DST = (uintptr_t)2 << 40, M01 = (uintptr_t)3 << 40;      // never dereferenced

static srgd_selfens_record record() {
  srgd_selfens_record r;
  std::memset(&r, 0, sizeof r);
  r.h = 7;
  r.w = 5;
  r.op = 5;
  return r;
}

static bool t_refused(const srgd_selfens_record* recs, int n, uintptr_t src, uintptr_t dst, const char* word) {
  const int rc = srgd_selfens_transform((const void*)src, (void*)dst, recs, n, nullptr);
  const bool ok = rc == -1 && std::strstr(srgd_selfens_last_error(), word) != nullptr &&
                  std::strncmp(srgd_selfens_last_error(), "srgd_selfens_transform", 22) == 0;
  if (!ok) std::printf("  transform: rc %d, message '%s', wanted '%s'\n", rc, srgd_selfens_last_error(), word);
  return ok;
}

static srgd_selfens_image image() {
  srgd_selfens_image m;
  std::memset(&m, 0, sizeof m);
  m.H = 7;
  m.W = 5;
  m.n_src = 2;
  m.src_off[1] = 112;
  m.op[1] = 5;
  for (int j = 2; j < 8; ++j) {                          // ignored: beyond n_src
    m.src_off[j] = -3;
    m.op[j] = 99;
  }
  return m;
}

static bool m_refused(const srgd_selfens_image* ims, int n, uintptr_t src, uintptr_t dst, uintptr_t m01, const char* word) {
  const int rc = srgd_selfens_merge((const void*)src, (void*)dst, (float*)m01, ims, n, nullptr);
  const bool ok = rc == -1 && std::strstr(srgd_selfens_last_error(), word) != nullptr &&
                  std::strncmp(srgd_selfens_last_error(), "srgd_selfens_merge", 18) == 0;
  if (!ok) std::printf("  merge: rc %d, message '%s', wanted '%s'\n", rc, srgd_selfens_last_error(), word);
  return ok;
}

int main() {
  EXPECT(sizeof(srgd_selfens_record) == 32 && sizeof(srgd_selfens_image) == 128);
  EXPECT(srgd_selfens_last_error() != nullptr);

  // ---- srgd_selfens_transform
  std::vector<srgd_selfens_record> one(1, record());
  EXPECT(t_refused(one.data(), 1, 0, DST, "null"));
  EXPECT(t_refused(one.data(), 1, SRC, 0, "null"));
  EXPECT(t_refused(nullptr, 1, SRC, DST, "null"));
  EXPECT(t_refused(one.data(), 0, SRC, DST, "n must be"));
  EXPECT(t_refused(one.data(), -5, SRC, DST, "n must be"));
  EXPECT(t_refused(one.data(), 1, SRC + 8, DST, "16-byte aligned"));
  EXPECT(t_refused(one.data(), 1, SRC, DST + 4, "16-byte aligned"));
  EXPECT(t_refused(one.data(), 1, SRC, SRC, "overlap"));
  EXPECT(t_refused(one.data(), 1, SRC, SRC + 96, "overlap"));
  struct Edit { int field; long long value; const char* word; };
  // field: 0 h, 1 w, 2 op, 3 src_off, 4 dst_off, 5 h and w.  "overlap" = the record itself passed (src == dst in these calls)
  const Edit edits[] = {{0, 0, "bad size"}, {1, -1, "bad size"}, {0, -2147483647 - 1, "bad size"}, {5, 26755, "bad size"}, {5, 26754, "overlap"},
                        {5, 2147483647, "bad size"}, {0, 143165577, "bad size"}, {0, 143165576, "overlap"}, {2, -1, "op outside"},
                        {2, 8, "op outside"}, {2, 0, "overlap"}, {2, 7, "overlap"}, {3, 8, "multiple of 16"}, {4, 17, "multiple of 16"},
                        {3, -16, "outside [0, 2^36)"}, {4, 1ll << 36, "outside [0, 2^36)"}, {4, (1ll << 36) - 16, "overlap"}, {3, 0, "overlap"}};
  for (const Edit& e : edits) {
    std::vector<srgd_selfens_record> recs(2, record());
    srgd_selfens_record& r = recs[1];                    // the second record: every record is checked before the first launch
    if (e.field == 0) r.h = (int32_t)e.value;
    if (e.field == 1) r.w = (int32_t)e.value;
    if (e.field == 2) r.op = (int32_t)e.value;
    if (e.field == 3) r.src_off = e.value;
    if (e.field == 4) r.dst_off = e.value;
    if (e.field == 5) r.h = r.w = (int32_t)e.value;
    EXPECT(t_refused(recs.data(), 2, SRC, SRC, e.word));
  }
  for (int op = -1; op <= 8; ++op) {
    one[0].op = op;
    EXPECT(t_refused(one.data(), 1, SRC, SRC, op < 0 || op > 7 ? "op outside" : "overlap"));
  }

  // ---- srgd_selfens_merge
  std::vector<srgd_selfens_image> im(1, image());
  EXPECT(m_refused(im.data(), 1, 0, DST, M01, "null"));
  EXPECT(m_refused(im.data(), 1, SRC, 0, 0, "null"));
  EXPECT(m_refused(nullptr, 1, SRC, DST, M01, "null"));
  EXPECT(m_refused(im.data(), 0, SRC, DST, M01, "n_images"));
  EXPECT(m_refused(im.data(), 1, SRC + 4, DST, M01, "16-byte aligned"));
  EXPECT(m_refused(im.data(), 1, SRC, DST + 8, M01, "16-byte aligned"));
  EXPECT(m_refused(im.data(), 1, SRC, DST, M01 + 2, "4-byte aligned"));
  EXPECT(m_refused(im.data(), 1, SRC, SRC, M01, "overlap"));
  EXPECT(m_refused(im.data(), 1, SRC, SRC + 208, 0, "overlap"));            // mean01 may be null; the last source ends at 112 + 105
  // field: 0 H, 1 W, 2 n_src, 3 op[1], 4 src_off[1], 5 dst_off, 6 mean01_off, 7 H and W, 8 op[7] with n_src = 8, 9 src_off[7] with n_src = 8
  const Edit medits[] = {{0, 0, "bad size"}, {1, -7, "bad size"}, {7, 26755, "bad size"}, {7, 26754, "overlap"}, {2, 0, "n_src"}, {2, 9, "n_src"},
                         {2, -1, "n_src"}, {2, 1, "overlap"}, {3, 8, "op outside"}, {3, -1, "op outside"}, {3, 7, "overlap"},
                         {4, 120, "multiple of 16"}, {4, -16, "outside [0, 2^36)"}, {4, 1ll << 36, "outside [0, 2^36)"},
                         {4, (1ll << 36) - 16, "overlap"}, {5, 24, "multiple of 16"}, {5, -16, "outside [0, 2^36)"}, {5, 1ll << 36, "outside [0, 2^36)"},
                         {6, -1, "negative mean01"}, {6, 3, "overlap"}, {8, 8, "op outside"}, {8, 6, "overlap"}, {9, 8, "multiple of 16"},
                         {9, 4096, "overlap"}};
  for (const Edit& e : medits) {
    std::vector<srgd_selfens_image> ims(2, image());
    srgd_selfens_image& m = ims[1];
    if (e.field >= 8) {
      m.n_src = 8;
      for (int j = 0; j < 8; ++j) {
        m.src_off[j] = 112 * j;
        m.op[j] = j;
      }
    }
    if (e.field == 0) m.H = (int32_t)e.value;
    if (e.field == 1) m.W = (int32_t)e.value;
    if (e.field == 2) m.n_src = (int32_t)e.value;
    if (e.field == 3) m.op[1] = (int32_t)e.value;
    if (e.field == 4) m.src_off[1] = e.value;
    if (e.field == 5) m.dst_off = e.value;
    if (e.field == 6) m.mean01_off = e.value;
    if (e.field == 7) m.H = m.W = (int32_t)e.value;
    if (e.field == 8) m.op[7] = (int32_t)e.value;
    if (e.field == 9) m.src_off[7] = e.value;
    EXPECT(m_refused(ims.data(), 2, SRC, SRC, M01, e.word));
  }
  {                                                      // a negative mean01 offset is not looked at where mean01 is NULL
    std::vector<srgd_selfens_image> ims(1, image());
    ims[0].mean01_off = -1;
    EXPECT(m_refused(ims.data(), 1, SRC, SRC, 0, "overlap"));
  }
  std::printf(failures ? "selfens_host_check: %d FAILED\n" : "selfens_host_check: ok (%d failures)\n", failures);
  return failures ? 1 : 0;
}
