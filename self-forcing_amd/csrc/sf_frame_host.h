// Internal scaffold shared by the frame and keypoint entry points (jpeg, jpeg_decode, resize, pose_render, pose_retarget,
// pose_smooth, pose_track, pose_estimate, pose_conv's sf_pose_prepare): what stands in front of kernels that index
// caller memory with no bounds of their own, written once.  Host-side only; not part of include/sf_hip.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/sf_hip.h"

// ---- layer 1, plain C++ (no HIP: tests/frame_host_main.cpp is a host program over it)
extern "C" void sf_set_error(const char* fmt, ...);

constexpr int POINTS = 134, BODY = 18;                  // a keypoint row [POINTS][3] of (x, y, score), the BODY points first
constexpr float ABSENT_XY = -1.f, ABSENT_SCORE = 0.f;   // a point that is not there

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// kZigzag[k] = natural index of the k-th coefficient of a JPEG scan
inline constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// element (f, c, y, x) of n frames of h x w in `layout` (enum sf_jpeg_layout, checked by the caller) stands at f sn + c sc + y sy + x sx
struct FrameStrides { long sn, sc, sy, sx; };
inline FrameStrides frame_strides(int layout, int n, int h, int w) {
  const long hw = (long)h * w;
  if (layout == SF_JPEG_HWC) return {3 * hw, 1, 3L * w, 3};
  if (layout == SF_JPEG_POSE) return {hw, (long)n * hw, w, 1};
  return {3 * hw, hw, w, 1};
}

// the byte ranges a call reads and writes; disjoint() refuses the first pair (i < j, in declaration order) that shares a byte
struct Range { const char* name; const void* p; size_t bytes; };
inline bool overlap(const Range& a, const Range& b) {
  const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
  return x < y + b.bytes && y < x + a.bytes;
}
template <int N>
inline int disjoint(const char* who, const Range (&r)[N]) {
  for (int i = 0; i < N; ++i)
    for (int j = i + 1; j < N; ++j)
      if (overlap(r[i], r[j])) return sf_set_error("%s: %s and %s overlap", who, r[i].name, r[j].name), -1;
  return 0;
}

// ---- layer 2: f(PixelType<T>{}) for the T that `dtype` (enum sf_jpeg_dtype, checked by the caller) names; a kernel
// that has no uint8 form says U8 = false
#ifdef __HIPCC__
#include "sf_host.h"
template <typename T> struct PixelType { using type = T; };
template <bool U8 = true, typename F>
inline int pixel_dispatch(int dtype, F&& f) {
  if constexpr (U8)
    if (dtype == SF_JPEG_U8) return f(PixelType<uint8_t>{});
  if (dtype == SF_JPEG_F32) return f(PixelType<float>{});
  return f(PixelType<bf16_t>{});
}
#endif
