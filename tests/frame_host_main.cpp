// Host program for the plain-C++ layer of self-forcing_amd/csrc/sf_frame_host.h (no HIP, no GPU):
//   c++ -std=c++17 -I self-forcing_amd/csrc tests/frame_host_main.cpp -o frame_host && ./frame_host
// tests/test_frame_host.py builds and runs it; with -fsanitize=address,undefined it is the memory check of that layer.
// sf_set_error is a stand-in that keeps the message, as capi.cpp does for the library.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "sf_frame_host.h"

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: FAILED %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static char last_error[256];
extern "C" void sf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(last_error, sizeof(last_error), fmt, ap);
  va_end(ap);
}

namespace {

// disjoint() over {a, b, c} at the given offsets and sizes inside one buffer: 0 and no message, or -1 and `message`
void expect_disjoint(const char* base, size_t a, size_t na, size_t b, size_t nb, size_t c, size_t nc, const char* message) {
  const Range r[3] = {{"a", base + a, na}, {"b", base + b, nb}, {"c", base + c, nc}};
  std::strcpy(last_error, "");
  const int rc = disjoint("who", r);
  EXPECT(rc == (message ? -1 : 0));
  EXPECT(std::strcmp(last_error, message ? message : "") == 0);
  if (std::strcmp(last_error, message ? message : "") != 0) std::fprintf(stderr, "  got \"%s\"\n", last_error);
}

void ranges() {
  static const char buf[256] = {};
  // end to start: [0, 16) [16, 32) [32, 48) share nothing
  expect_disjoint(buf, 0, 16, 16, 16, 32, 16, nullptr);
  // one shared byte: b starts on a's last byte; b and c, c and a
  expect_disjoint(buf, 0, 16, 15, 16, 64, 16, "who: a and b overlap");
  expect_disjoint(buf, 0, 16, 32, 16, 47, 16, "who: b and c overlap");
  expect_disjoint(buf, 31, 16, 64, 16, 16, 16, "who: a and c overlap");
  // nested: c inside a, a inside c
  expect_disjoint(buf, 0, 64, 128, 16, 8, 8, "who: a and c overlap");
  expect_disjoint(buf, 8, 8, 128, 16, 0, 64, "who: a and c overlap");
  // reversed address order: disjoint stays disjoint, end to start included
  expect_disjoint(buf, 32, 16, 16, 16, 0, 16, nullptr);
  expect_disjoint(buf, 32, 16, 16, 17, 0, 16, "who: a and b overlap");
  expect_disjoint(buf, 64, 16, 16, 16, 0, 17, "who: b and c overlap");
  // the first pair in i < j order is named: a overlaps both, b and c overlap too
  expect_disjoint(buf, 0, 64, 8, 16, 16, 16, "who: a and b overlap");
  expect_disjoint(buf, 0, 8, 8, 16, 4, 16, "who: a and c overlap");
  // overlap() itself is symmetric
  const Range x = {"x", buf, 16}, y = {"y", buf + 15, 1}, z = {"z", buf + 16, 1};
  EXPECT(overlap(x, y) && overlap(y, x) && !overlap(x, z) && !overlap(z, x) && overlap(x, x));
}

void expect_strides(int layout, long sn, long sc, long sy, long sx) {
  const FrameStrides s = frame_strides(layout, 2, 3, 5);
  EXPECT(s.sn == sn && s.sc == sc && s.sy == sy && s.sx == sx);
}

void strides() {
  // n = 2 frames of h = 3, w = 5
  expect_strides(SF_JPEG_HWC, 45, 1, 15, 3);    // [n][h][w][3]
  expect_strides(SF_JPEG_POSE, 15, 30, 5, 1);   // [3][n][h][w]: a channel is n * h * w elements
  expect_strides(SF_JPEG_CHW, 45, 15, 5, 1);    // [n][3][h][w]
  // the products are formed in 64 bits
  EXPECT(frame_strides(SF_JPEG_POSE, 65535, 65535, 65535).sc == 65535L * 65535L * 65535L);
}

void constants() {
  EXPECT(POINTS == 134 && BODY == 18 && ABSENT_XY == -1.f && ABSENT_SCORE == 0.f);
  bool seen[64] = {};
  for (int k = 0; k < 64; ++k) seen[kZigzag[k]] = true;
  for (int i = 0; i < 64; ++i) EXPECT(seen[i]);                     // a permutation of 0..63
  EXPECT(kZigzag[1] == 1 && kZigzag[2] == 8 && kZigzag[63] == 63);
  EXPECT(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
}

}  // namespace

int main() {
  ranges();
  strides();
  constants();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("frame host: all checks passed");
  return 0;
}
