// Raw YUV frames <-> RGB frames (gfx950): the pixel formats video has outside JPEG -- planar i420 / i422 / i444, semi-planar
// nv12, packed yuyv / uyvy, gray -- cross the border of the device as they are, 1.5 or 2 bytes per pixel.  The definition
// of every number is self_forcing_amd/yuv_reference.py (`decode`, `encode`); the caller computes the sixteen constants with
// `yuv_reference.constants` and passes them as host memory, so the library holds no colour matrix of its own.
//
// yuv_to_rgb   one launch for all frames; a workgroup of 256 lanes takes a 16 x 64 tile, a lane four neighbouring pixels of
//              a row.  The host describes a format by offsets and strides (where sample (y, x) of Y and of U / V stands in a
//              frame), so the kernel has one body for all seven.  Luma, and chroma that is not subsampled, is one dword load
//              where the address is 4-byte aligned (frame_bytes may be odd, so that depends on the frame) and byte loads
//              where it is not; subsampled chroma is read as bytes (nv12: as U V pairs where the frame starts even)
//              straight from global memory: the triangle filter's 2 x 4 neighbourhood starts at an odd column, so no aligned
//              vector covers it, and the lanes of a wave that share a sample hit the same cache line.
//              The output goes through pixel_format.h.
// rgb_to_yuv   one launch for all frames; a lane owns 8 x 2 pixels: every pixel is converted at full resolution, the block
//              yields two runs of eight luma bytes and whole chroma samples for every subsampling (4 U and 4 V for i420 /
//              nv12).  Vector loads and stores where whole and aligned, bytes at the edges and in unaligned frames.
// No workspace, no state; every index is clamped to the plane it reads, every store guarded by the frame's size.
#include "sf_frame_host.h"
#include "pixel_format.h"

namespace {

constexpr int TW = 64, TH = 16;          // decode tile: 256 lanes = TH rows x TW / 4 quads
constexpr int EW = 8, EH = 2;            // encode: pixels of one lane; a workgroup is 16 x 16 lanes

struct YuvDecodeArgs {
  const uint8_t* raw;
  long frame_bytes;
  int h, w, ch, cw;                      // frame and chroma plane size
  long y_off, c_off[2];                  // byte offset of Y(0, 0), U(0, 0), V(0, 0) in a frame
  int y_row, y_step, c_row, c_step;      // byte strides of a luma / chroma row and column
  int sub_x, sub_y;                      // 1 where chroma has half the columns / rows
  int triangle, gray;
  int k[6];                              // yoff, CY, CRV, CGU, CGV, CBU
  long sn, sc, sy, sx;                   // element strides of the output
};

struct YuvEncodeArgs {
  long in_sn, in_sc, in_sy, in_sx;       // element strides of the input
  long frame_bytes;
  int h, w, ch, cw;
  long c_off[2];
  int c_row, c_step;
  int sub_x, sub_y;
  int range01;
  int k[10];                             // yoff, YR, YG, YB, UR, UG, UB, VR, VG, VB
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// four bytes next to each other, the ones at index >= count replaced by the last valid one
__device__ __forceinline__ void load_run4(const uint8_t* p, int count, int (&v)[4]) {
  if (count >= 4 && ((uintptr_t)p & 3) == 0) {
    const uint32_t d = *(const uint32_t*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (int)((d >> (8 * i)) & 255u);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = p[min(i, count - 1)];
  }
}

// grid (ceil(w / TW), ceil(h / TH), n)
template <typename T>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const YuvDecodeArgs a, T* __restrict__ out) {
  const int t = threadIdx.x, q = t & 15, ty = t >> 4;
  const int x0 = blockIdx.x * TW + 4 * q, y = blockIdx.y * TH + ty;
  const long f = blockIdx.z;
  if (y >= a.h || x0 >= a.w) return;
  const uint8_t* fr = a.raw + f * a.frame_bytes;
  const int count = min(4, a.w - x0);

  int Y[4];
  if (a.y_step == 1) {
    load_run4(fr + a.y_off + (long)y * a.y_row + x0, count, Y);
  } else {                                                         // packed: Y U Y V or U Y V Y, eight bytes of a quad
    const uint8_t* p = fr + (long)y * a.y_row + 2L * x0;
    if (count == 4 && ((uintptr_t)p & 3) == 0) {
      const uint32_t d0 = ((const uint32_t*)p)[0], d1 = ((const uint32_t*)p)[1];
      const int sh = 8 * (int)a.y_off;
      Y[0] = (d0 >> sh) & 255u, Y[1] = (d0 >> (sh + 16)) & 255u, Y[2] = (d1 >> sh) & 255u, Y[3] = (d1 >> (sh + 16)) & 255u;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) Y[i] = p[a.y_off + 2 * min(i, count - 1)];
    }
  }

  int C[2][4];
  if (a.gray) {
#pragma unroll
    for (int i = 0; i < 4; ++i) C[0][i] = C[1][i] = 128;
  } else if (!a.sub_x) {                                           // i444: the luma's geometry
#pragma unroll
    for (int c = 0; c < 2; ++c) load_run4(fr + a.c_off[c] + (long)y * a.c_row + x0, count, C[c]);
  } else {
    const int cx0 = x0 >> 1, cya = y >> a.sub_y;
    const bool vert = a.triangle && a.sub_y;
    const int cyb = vert ? ((y & 1) ? min(cya + 1, a.ch - 1) : max(cya - 1, 0)) : cya;
    int col[4];                                                    // triangle: cx0 - 1 .. cx0 + 2; nearest: cx0, cx0, cx0 + 1, cx0 + 1
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = clampi(a.triangle ? cx0 - 1 + j : cx0 + (j >> 1), 0, a.cw - 1) * a.c_step;
    int s2[2][4];
    const uint8_t* c0 = fr + a.c_off[0];
    if (a.c_step == 2 && a.c_off[1] == a.c_off[0] + 1 && ((uintptr_t)c0 & 1) == 0) {   // nv12 in an even frame: U and V in one load
      const uint8_t* pa = c0 + (long)cya * a.c_row;
      const uint8_t* pb = c0 + (long)cyb * a.c_row;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int va = *(const uint16_t*)(pa + col[j]);
        s2[0][j] = va & 255, s2[1][j] = va >> 8;
        if (vert) {
          const int vb = *(const uint16_t*)(pb + col[j]);
          s2[0][j] = 3 * s2[0][j] + (vb & 255), s2[1][j] = 3 * s2[1][j] + (vb >> 8);
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const uint8_t* pa = fr + a.c_off[c] + (long)cya * a.c_row;
        const uint8_t* pb = fr + a.c_off[c] + (long)cyb * a.c_row;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s2[c][j] = pa[col[j]];
          if (vert) s2[c][j] = 3 * s2[c][j] + pb[col[j]];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int(&s)[4] = s2[c];
      if (!a.triangle) {
#pragma unroll
        for (int j = 0; j < 4; ++j) C[c][j] = s[j];
      } else if (vert) {                                           // jpeg_reference.upsample, 2 x 2
        C[c][0] = (3 * s[1] + s[0] + 8) >> 4, C[c][1] = (3 * s[1] + s[2] + 7) >> 4;
        C[c][2] = (3 * s[2] + s[1] + 8) >> 4, C[c][3] = (3 * s[2] + s[3] + 7) >> 4;
      } else {                                                     // 2 x 1
        C[c][0] = (3 * s[1] + s[0] + 1) >> 2, C[c][1] = (3 * s[1] + s[2] + 2) >> 2;
        C[c][2] = (3 * s[2] + s[1] + 1) >> 2, C[c][3] = (3 * s[2] + s[3] + 2) >> 2;
      }
    }
  }

  int rgb[3][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int yv = (Y[i] - a.k[0]) * a.k[1] + 32768, cb = C[0][i] - 128, cr = C[1][i] - 128;
    rgb[0][i] = clamp255((yv + a.k[2] * cr) >> 16);
    rgb[1][i] = clamp255((yv - a.k[3] * cb - a.k[4] * cr) >> 16);
    rgb[2][i] = clamp255((yv + a.k[5] * cb) >> 16);
  }
  T* o = out + f * a.sn + (long)y * a.sy + (long)x0 * a.sx;
  store_rgb4(o, rgb, x0, a.w, a.sc, a.sx);
}

// jpeg.hip's conversion of a float sample to 8 bit (jpeg_reference.to_uint8): the multiply and the add each rounded
__device__ __forceinline__ int to_u8(float p, int range01) {
#pragma clang fp contract(off)
  if (range01) return (int)truncf(255.f * fminf(fmaxf(p, 0.f), 1.f));
  const float scaled = fminf(fmaxf(p, -1.f), 1.f) * 127.5f;
  return (int)truncf(scaled + 127.5f);
}

__device__ __forceinline__ float as_float(float v) { return v; }
__device__ __forceinline__ float as_float(bf16_t v) { return bf2f(v); }

// eight samples of one channel of one row, columns past the frame's last replaced by it
template <typename T>
__device__ __forceinline__ void load_row8(const T* p, int count, int range01, int (&v)[EW]) {
  if (count == EW && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 lo = ((const f32x4*)p)[0], hi = ((const f32x4*)p)[1];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = to_u8(lo[i], range01), v[4 + i] = to_u8(hi[i], range01);
    } else {
      const bf16x4 lo = ((const bf16x4*)p)[0], hi = ((const bf16x4*)p)[1];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = to_u8(bf2f(lo[i]), range01), v[4 + i] = to_u8(bf2f(hi[i]), range01);
    }
  } else {
#pragma unroll
    for (int i = 0; i < EW; ++i) v[i] = to_u8(as_float(p[min(i, count - 1)]), range01);
  }
}

// `count` (1..8) bytes of v to p: dwords where whole and aligned
__device__ __forceinline__ void store_run8(uint8_t* p, const int (&v)[EW], int count) {
  if (count == EW && ((uintptr_t)p & 3) == 0) {
#pragma unroll
    for (int d = 0; d < 2; ++d)
      ((uint32_t*)p)[d] = (uint32_t)v[4 * d] | ((uint32_t)v[4 * d + 1] << 8) | ((uint32_t)v[4 * d + 2] << 16) | ((uint32_t)v[4 * d + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < EW; ++i)
      if (i < count) p[i] = (uint8_t)v[i];
  }
}

// grid (ceil(w / (16 EW)), ceil(h / (16 EH)), n).  T = uint8_t: [n][h][w][3]; float / bf16_t: [n][3][h][w]
template <typename T>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const YuvEncodeArgs a, const T* __restrict__ in, uint8_t* __restrict__ out) {
  const int t = threadIdx.x;
  const int x0 = (blockIdx.x * 16 + (t & 15)) * EW, y0 = (blockIdx.y * 16 + (t >> 4)) * EH;
  const long f = blockIdx.z;
  if (x0 >= a.w || y0 >= a.h) return;
  const int count = min(EW, a.w - x0), rows = min(EH, a.h - y0);
  uint8_t* fr = out + f * a.frame_bytes;

  int Y[EH][EW], U[EH][EW], V[EH][EW];
#pragma unroll
  for (int r = 0; r < EH; ++r) {
    const int yy = min(y0 + r, a.h - 1);                           // a missing row is the last one again
    const T* p = in + f * a.in_sn + (long)yy * a.in_sy + (long)x0 * a.in_sx;
    int px[3][EW];
    if constexpr (sizeof(T) == 1) {
      if (count == EW && ((uintptr_t)p & 3) == 0) {                // 24 bytes R G B R G B ..
        uint32_t d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = ((const uint32_t*)p)[i];
#pragma unroll
        for (int i = 0; i < 24; ++i) px[i % 3][i / 3] = (int)((d[i >> 2] >> (8 * (i & 3))) & 255u);
      } else {
#pragma unroll
        for (int i = 0; i < EW; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c) px[c][i] = p[3 * min(i, count - 1) + c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) load_row8(p + c * a.in_sc, count, a.range01, px[c]);
    }
#pragma unroll
    for (int i = 0; i < EW; ++i) {
      const int R = px[0][i], G = px[1][i], B = px[2][i];
      Y[r][i] = clamp255((a.k[1] * R + a.k[2] * G + a.k[3] * B + (a.k[0] << 16) + 32768) >> 16);
      U[r][i] = clamp255((-a.k[4] * R - a.k[5] * G + a.k[6] * B + (128 << 16) + 32767) >> 16);
      V[r][i] = clamp255((a.k[7] * R - a.k[8] * G - a.k[9] * B + (128 << 16) + 32767) >> 16);
    }
  }

#pragma unroll
  for (int r = 0; r < EH; ++r)
    if (r < rows) store_run8(fr + (long)(y0 + r) * a.w + x0, Y[r], count);

  if (!a.sub_x) {                                                  // i444
#pragma unroll
    for (int r = 0; r < EH; ++r)
      if (r < rows) {
        store_run8(fr + a.c_off[0] + (long)(y0 + r) * a.c_row + x0, U[r], count);
        store_run8(fr + a.c_off[1] + (long)(y0 + r) * a.c_row + x0, V[r], count);
      }
    return;
  }
  const int cx0 = x0 >> 1, ccount = min(EW / 2, a.cw - cx0);
  const int crows = a.sub_y ? 1 : rows;
#pragma unroll
  for (int r = 0; r < EH; ++r) {
    if (r >= crows) continue;
    int cu[EW / 2], cv[EW / 2];
#pragma unroll
    for (int j = 0; j < EW / 2; ++j) {
      if (a.sub_y) {
        cu[j] = (U[0][2 * j] + U[0][2 * j + 1] + U[1][2 * j] + U[1][2 * j + 1] + 2) >> 2;
        cv[j] = (V[0][2 * j] + V[0][2 * j + 1] + V[1][2 * j] + V[1][2 * j + 1] + 2) >> 2;
      } else {
        cu[j] = (U[r][2 * j] + U[r][2 * j + 1] + 1) >> 1;
        cv[j] = (V[r][2 * j] + V[r][2 * j + 1] + 1) >> 1;
      }
    }
    const long row = (long)((a.sub_y ? y0 >> 1 : y0 + r)) * a.c_row;
    if (a.c_step == 2) {                                           // nv12: U V U V ..
      int uv[EW];
#pragma unroll
      for (int j = 0; j < EW / 2; ++j) uv[2 * j] = cu[j], uv[2 * j + 1] = cv[j];
      store_run8(fr + a.c_off[0] + row + 2L * cx0, uv, ccount == EW / 2 ? EW : 2 * ccount);
    } else {
      uint8_t* pu = fr + a.c_off[0] + row + cx0;
      uint8_t* pv = fr + a.c_off[1] + row + cx0;
      if (ccount == EW / 2 && (((uintptr_t)pu | (uintptr_t)pv) & 3) == 0) {
        *(uint32_t*)pu = (uint32_t)cu[0] | ((uint32_t)cu[1] << 8) | ((uint32_t)cu[2] << 16) | ((uint32_t)cu[3] << 24);
        *(uint32_t*)pv = (uint32_t)cv[0] | ((uint32_t)cv[1] << 8) | ((uint32_t)cv[2] << 16) | ((uint32_t)cv[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < EW / 2; ++j)
          if (j < ccount) pu[j] = (uint8_t)cu[j], pv[j] = (uint8_t)cv[j];
      }
    }
  }
}

// where a format keeps its samples; false = unknown format
struct YuvGeometry {
  long frame_bytes, y_off, c_off[2];
  int ch, cw, y_row, y_step, c_row, c_step, sub_x, sub_y, gray;
};
bool yuv_geometry(int format, int h, int w, YuvGeometry& g) {
  const long hw = (long)h * w;
  const int ch2 = (h + 1) / 2, cw2 = (w + 1) / 2;
  g = YuvGeometry{};
  g.y_row = w, g.y_step = 1, g.c_step = 1;
  switch (format) {
    case SF_YUV_I420: g.ch = ch2, g.cw = cw2, g.sub_x = g.sub_y = 1, g.c_row = cw2, g.c_off[0] = hw, g.c_off[1] = hw + (long)ch2 * cw2; break;
    case SF_YUV_NV12: g.ch = ch2, g.cw = cw2, g.sub_x = g.sub_y = 1, g.c_row = 2 * cw2, g.c_step = 2, g.c_off[0] = hw, g.c_off[1] = hw + 1; break;
    case SF_YUV_I422: g.ch = h, g.cw = cw2, g.sub_x = 1, g.c_row = cw2, g.c_off[0] = hw, g.c_off[1] = hw + (long)h * cw2; break;
    case SF_YUV_I444: g.ch = h, g.cw = w, g.c_row = w, g.c_off[0] = hw, g.c_off[1] = 2 * hw; break;
    case SF_YUV_GRAY: g.ch = h, g.cw = w, g.gray = 1, g.frame_bytes = hw; return true;
    case SF_YUV_YUYV:
    case SF_YUV_UYVY: {
      const int u = format == SF_YUV_YUYV;
      g.ch = h, g.cw = w / 2, g.sub_x = 1, g.y_row = g.c_row = 2 * w, g.y_step = 2, g.c_step = 4;
      g.y_off = u ? 0 : 1, g.c_off[0] = u ? 1 : 0, g.c_off[1] = u ? 3 : 2, g.frame_bytes = 2 * hw;
      return true;
    }
    default: return false;
  }
  g.frame_bytes = hw + 2L * g.ch * g.cw;
  return true;
}

int check_frame(const char* who, int format, int h, int w) {
  SF_CHECK(format >= SF_YUV_I420 && format <= SF_YUV_UYVY, "%s: unknown format %d", who, format);
  SF_CHECK(h > 0 && w > 0 && h <= SF_YUV_MAX_SIZE && w <= SF_YUV_MAX_SIZE, "%s: frame %dx%d (1..%d)", who, h, w, SF_YUV_MAX_SIZE);
  SF_CHECK((format != SF_YUV_YUYV && format != SF_YUV_UYVY) || w % 2 == 0, "%s: a packed 4:2:2 frame needs an even width, got %d", who, w);
  return 0;
}

}  // namespace

extern "C" size_t sf_yuv_frame_bytes(int format, int h, int w) {
  YuvGeometry g;
  if (check_frame("sf_yuv_frame_bytes", format, h, w) != 0 || !yuv_geometry(format, h, w, g)) return 0;
  return (size_t)g.frame_bytes;
}

extern "C" int sf_yuv_decode_frames(const void* raw, int format, int n, int h, int w, const int32_t* constants, int chroma, void* out, int layout, int dtype,
                                    void* stream) {
  const char* who = "sf_yuv_decode_frames";
  SF_CHECK(raw && out && constants, "%s: null buffer", who);
  SF_TRY(check_frame(who, format, h, w));
  SF_CHECK(chroma == SF_YUV_NEAREST || chroma == SF_YUV_TRIANGLE, "%s: unknown chroma filter %d", who, chroma);
  SF_CHECK(layout >= SF_JPEG_HWC && layout <= SF_JPEG_CHW, "%s: unknown layout %d", who, layout);
  SF_CHECK(dtype >= SF_JPEG_U8 && dtype <= SF_JPEG_BF16, "%s: unknown dtype %d", who, dtype);
  SF_CHECK(n > 0 && n <= 65535, "%s: n=%d frames (1..65535)", who, n);
  SF_CHECK((uintptr_t)out % 16 == 0, "%s: out must be 16-byte aligned", who);
  YuvGeometry g;
  yuv_geometry(format, h, w, g);
  const Range ranges[] = {{"raw", raw, (size_t)n * g.frame_bytes}, {"out", out, (size_t)n * 3 * h * w * (dtype == SF_JPEG_U8 ? 1 : dtype == SF_JPEG_F32 ? 4 : 2)}};
  SF_TRY(disjoint(who, ranges));
  YuvDecodeArgs a;
  a.raw = (const uint8_t*)raw, a.frame_bytes = g.frame_bytes;
  a.h = h, a.w = w, a.ch = g.ch, a.cw = g.cw;
  a.y_off = g.y_off, a.c_off[0] = g.c_off[0], a.c_off[1] = g.c_off[1];
  a.y_row = g.y_row, a.y_step = g.y_step, a.c_row = g.c_row, a.c_step = g.c_step;
  a.sub_x = g.sub_x, a.sub_y = g.sub_y, a.triangle = chroma == SF_YUV_TRIANGLE, a.gray = g.gray;
  for (int i = 0; i < 6; ++i) a.k[i] = constants[i];
  const FrameStrides to = frame_strides(layout, n, h, w);
  a.sn = to.sn, a.sc = to.sc, a.sy = to.sy, a.sx = to.sx;
  const dim3 grid((unsigned)((w + TW - 1) / TW), (unsigned)((h + TH - 1) / TH), (unsigned)n);
  hipStream_t s = (hipStream_t)stream;
  return pixel_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return sf_launch<&yuv_to_rgb_kernel<T>>(who, grid, dim3(256), 0, s, a, (T*)out);
  });
}

extern "C" int sf_yuv_encode_frames(const void* frames, int dtype, int value_range, int n, int h, int w, const int32_t* constants, void* out, int format,
                                    void* stream) {
  const char* who = "sf_yuv_encode_frames";
  SF_CHECK(frames && out && constants, "%s: null buffer", who);
  SF_TRY(check_frame(who, format, h, w));
  SF_CHECK(format <= SF_YUV_I444, "%s: format %d is decode only (the encoder writes i420, nv12, i422, i444)", who, format);
  SF_CHECK(dtype >= SF_JPEG_U8 && dtype <= SF_JPEG_BF16, "%s: unknown dtype %d", who, dtype);
  SF_CHECK(value_range == SF_JPEG_RANGE_PM1 || value_range == SF_JPEG_RANGE_01, "%s: unknown value range %d", who, value_range);
  SF_CHECK(n > 0 && n <= 65535, "%s: n=%d frames (1..65535)", who, n);
  const size_t esize = dtype == SF_JPEG_U8 ? 1 : dtype == SF_JPEG_F32 ? 4 : 2;
  SF_CHECK((uintptr_t)frames % esize == 0, "%s: frames must be aligned to their element", who);
  YuvGeometry g;
  yuv_geometry(format, h, w, g);
  const Range ranges[] = {{"frames", frames, (size_t)n * 3 * h * w * esize}, {"out", out, (size_t)n * g.frame_bytes}};
  SF_TRY(disjoint(who, ranges));
  YuvEncodeArgs a;
  const FrameStrides in = frame_strides(dtype == SF_JPEG_U8 ? SF_JPEG_HWC : SF_JPEG_CHW, n, h, w);
  a.in_sn = in.sn, a.in_sc = in.sc, a.in_sy = in.sy, a.in_sx = in.sx;
  a.frame_bytes = g.frame_bytes, a.h = h, a.w = w, a.ch = g.ch, a.cw = g.cw;
  a.c_off[0] = g.c_off[0], a.c_off[1] = g.c_off[1], a.c_row = g.c_row, a.c_step = g.c_step, a.sub_x = g.sub_x, a.sub_y = g.sub_y;
  a.range01 = value_range == SF_JPEG_RANGE_01;
  a.k[0] = constants[0];
  for (int i = 1; i < 10; ++i) a.k[i] = constants[5 + i];
  const dim3 grid((unsigned)((w + 16 * EW - 1) / (16 * EW)), (unsigned)((h + 16 * EH - 1) / (16 * EH)), (unsigned)n);
  hipStream_t s = (hipStream_t)stream;
  return pixel_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return sf_launch<&rgb_to_yuv_kernel<T>>(who, grid, dim3(256), 0, s, a, (const T*)frames, (uint8_t*)out);
  });
}
