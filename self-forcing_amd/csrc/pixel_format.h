// 8-bit samples into the output types of the frame kernels (jpeg_decode.hip, resize.hip): one definition of
// u8 / 127.5 - 1, so that the decoder's and the resizer's float frames agree to the bit.
#pragma once
#include "sf_common.h"

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// u8 / 127.5 - 1, the divide and the subtract each rounded to fp32 (jpeg_reference.to_float)
__device__ __forceinline__ float to_pm1(int v) {
#pragma clang fp contract(off)
  const float q = (float)v / 127.5f;
  return q - 1.0f;
}

__device__ __forceinline__ void convert(int v, uint8_t& o) { o = (uint8_t)v; }
__device__ __forceinline__ void convert(int v, float& o) { o = to_pm1(v); }
__device__ __forceinline__ void convert(int v, bf16_t& o) { o = f2bf(to_pm1(v)); }

// four values next to each other, 4 sizeof(T)-aligned
__device__ __forceinline__ void store4(uint8_t* p, const int (&v)[4]) {
  *(uint32_t*)p = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}
__device__ __forceinline__ void store4(float* p, const int (&v)[4]) { *(f32x4*)p = f32x4{to_pm1(v[0]), to_pm1(v[1]), to_pm1(v[2]), to_pm1(v[3])}; }
__device__ __forceinline__ void store4(bf16_t* p, const int (&v)[4]) {
  *(bf16x4*)p = bf16x4{f2bf(to_pm1(v[0])), f2bf(to_pm1(v[1])), f2bf(to_pm1(v[2])), f2bf(to_pm1(v[3]))};
}

// Four pixels (x0 .. x0 + 3 of one row, the columns >= W dropped) of three channels into a frame whose element (c, x)
// stands at o[c * sc + x * sx]: whole quads as vector stores where the layout has them aligned, single elements otherwise.
template <typename T>
__device__ __forceinline__ void store_rgb4(T* o, const int (&rgb)[3][4], int x0, int W, long sc, long sx) {
  if (sx == 1 && (W & 3) == 0) {                                   // planar rows of whole quads
#pragma unroll
    for (int c = 0; c < 3; ++c) store4(o + c * sc, rgb[c]);
  } else if (sizeof(T) == 1 && sx == 3 && sc == 1 && (W & 3) == 0) {         // uint8 [.., W, 3]: twelve bytes
    uint32_t w[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i >> 2] |= (uint32_t)rgb[i % 3][i / 3] << (8 * (i & 3));
#pragma unroll
    for (int i = 0; i < 3; ++i) ((uint32_t*)o)[i] = w[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x0 + i < W)
#pragma unroll
        for (int c = 0; c < 3; ++c) convert(rgb[c][i], o[c * sc + i * sx]);
  }
}
