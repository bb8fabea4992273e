// Frame resizer (gfx950): uint8 frames change their size on the device, with the bits of Pillow's 8-bit resampler
// (Image.resize with BILINEAR or BICUBIC: antialiased, 22-bit fixed-point coefficients, a horizontal pass rounded to
// uint8, then a vertical pass over that result).  The definition of every number is self_forcing_amd/resize_reference.py
// (`coefficients`, `resize`); the caller builds the two coefficient tables with it and passes them as device memory, so
// the double-precision arithmetic exists once.
//
// One fused kernel, one workgroup of 256 threads per output tile of TH x TW pixels of one frame:
//   stage 0  the tile's rows of both tables go to LDS, bounds clamped to the crop and to the table's width
//   stage 1  the input rows [Y0, Y0 + R) the tile's vertical taps reach are resampled horizontally, `rb` rows at a time:
//            the bytes of the columns [X0, X0 + ncols) are fetched as whole aligned dwords into LDS (one contiguous run
//            per row for [h][w][3], three for the planar layouts), then each thread forms one pixel of one row, three
//            channels, from LDS bytes and writes it as uint8 into the LDS intermediate [3][R][TW]
//   stage 2  each thread resamples four neighbouring columns of one output row vertically (one LDS dword per tap and
//            channel) and stores them in the requested layout and type
// The intermediate never reaches memory; rows that vertically adjacent tiles share are resampled once per tile.
// LDS grows with the reduction ratio; at SF_RESIZE_MAX_RATIO per axis it is 58 KiB, which is where the limit comes from.
// Nothing in the tables is trusted: every LDS index derived from them is checked against the tile's extent, every
// global read lies inside the frames, every write inside the output tile.
#include "sf_frame_host.h"
#include "pixel_format.h"

namespace {

constexpr int TW = 64, TH = 16;          // output tile; 256 threads = TH rows x TW / 4 quads in stage 2
constexpr int IST = TW + 4;              // row stride of the intermediate (bytes): 17 dwords, rows fall on different banks
constexpr int PRECISION_BITS = 22;
constexpr int STAGE_BYTES = 16384;       // target size of stage 1's input rows in LDS

struct ResizeArgs {
  const uint8_t* in;
  long in_bytes;                         // n * h * w * 3
  long in_sn, in_sc, in_sy, in_sx;       // byte strides of the input's frame, channel, row, column
  int top, left, ch, cw;                 // the crop
  const int32_t *bh, *kh, *bv, *kv;      // bounds [out][2] and coefficients [out][ks] of the horizontal and the vertical pass
  int ksh, ksv;
  int oh, ow;
  long sn, sc, sy, sx;                   // element strides of the output
  int caph, capv;                        // the most columns / rows of the input one tile reaches
  int rb, nseg, seg_stride;              // stage 1: rows per batch, runs per row, bytes of one run's LDS slot
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T>
__global__ __launch_bounds__(256) void resize_kernel(ResizeArgs a, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  int* s_bh = (int*)lds;
  int* s_kh = s_bh + 2 * TW;
  int* s_bv = s_kh + TW * a.ksh;
  int* s_kv = s_bv + 2 * TH;
  uint8_t* inter = (uint8_t*)(s_kv + TH * a.ksv);
  uint8_t* stage = inter + ((3 * a.capv * IST + 3) & ~3);

  const int t = threadIdx.x;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
  const long f = blockIdx.z;
  const int tw = min(TW, a.ow - ox0), th = min(TH, a.oh - oy0);

  // ---- stage 0: the tile's table rows
  for (int i = t; i < TW + TH; i += 256) {
    const bool hor = i < TW;
    const int j = hor ? i : i - TW, cnt = hor ? tw : th, size = hor ? a.cw : a.ch, ks = hor ? a.ksh : a.ksv;
    const int32_t* b = hor ? a.bh + 2L * ox0 : a.bv + 2L * oy0;
    int lo = 0, num = 0;
    if (j < cnt) {
      lo = clampi(b[2 * j], 0, size - 1);
      num = clampi(b[2 * j + 1], 0, min(ks, size - lo));
    }
    int* s = hor ? s_bh : s_bv;
    s[2 * j] = lo, s[2 * j + 1] = num;
  }
  for (int i = t; i < tw * a.ksh; i += 256) s_kh[i] = a.kh[(long)ox0 * a.ksh + i];
  for (int i = t; i < th * a.ksv; i += 256) s_kv[i] = a.kv[(long)oy0 * a.ksv + i];
  __syncthreads();

  const int X0 = s_bh[0], Y0 = s_bv[0];
  const int ncols = clampi(s_bh[2 * (tw - 1)] + s_bh[2 * (tw - 1) + 1] - X0, 0, min(a.caph, a.cw - X0));
  const int R = clampi(s_bv[2 * (th - 1)] + s_bv[2 * (th - 1) + 1] - Y0, 0, min(a.capv, a.ch - Y0));
  const int seg_bytes = ncols * (a.nseg == 1 ? 3 : 1);
  const int slot_dwords = a.seg_stride >> 2;
  // byte offset of run `s` of tile row `r` in the input
  auto run_start = [&](int r, int s) -> long {
    return f * a.in_sn + (long)(a.top + Y0 + r) * a.in_sy + (long)(a.left + X0) * a.in_sx + (a.nseg == 3 ? s * a.in_sc : 0);
  };

  // ---- stage 1: horizontal pass into the intermediate, rb rows at a time
  for (int r0 = 0; r0 < R; r0 += a.rb) {
    const int nb = min(a.rb, R - r0);
    for (int idx = t; idx < nb * a.nseg * slot_dwords; idx += 256) {
      const int rs = idx / slot_dwords, d = idx - rs * slot_dwords;
      const int r = rs / a.nseg, s = rs - r * a.nseg;
      const long g = run_start(r0 + r, s), a0 = g & ~3L;
      if (4L * d < g + seg_bytes - a0) {
        const long at = a0 + 4L * d;
        uint32_t v = 0;
        if (at + 4 <= a.in_bytes) {
          v = *(const uint32_t*)(a.in + at);
        } else {                                                   // the frames' last bytes: no read behind them
          for (int b = 0; b < 4; ++b)
            if (at + b < a.in_bytes) v |= (uint32_t)a.in[at + b] << (8 * b);
        }
        *(uint32_t*)(stage + (long)rs * a.seg_stride + 4 * d) = v;
      }
    }
    __syncthreads();
    for (int item = t; item < nb * TW; item += 256) {
      const int rl = item / TW, x = item - rl * TW;
      int px[3] = {0, 0, 0};
      if (x < tw) {
        const int first = s_bh[2 * x] - X0, num = s_bh[2 * x + 1];
        const int* k = s_kh + x * a.ksh;
        const uint8_t* p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int s = a.nseg == 3 ? c : 0;
          p[c] = stage + (long)(rl * a.nseg + s) * a.seg_stride + (int)(run_start(r0 + rl, s) & 3) + (a.nseg == 1 ? c : 0);
        }
        int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
        const int step = (int)a.in_sx;
        for (int i = 0; i < num; ++i) {
          const int col = first + i;
          if ((unsigned)col < (unsigned)ncols) {
            const int w = k[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += (int)p[c][col * step] * w;
          }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = clamp255(acc[c] >> PRECISION_BITS);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) inter[(c * a.capv + r0 + rl) * IST + x] = (uint8_t)px[c];
    }
    __syncthreads();
  }

  // ---- stage 2: vertical pass, four columns of one row per thread
  const int ty = t >> 4, q = t & 15;
  if (ty >= th || 4 * q >= tw) return;
  const int first = s_bv[2 * ty] - Y0, num = s_bv[2 * ty + 1];
  const int* k = s_kv + ty * a.ksv;
  int acc[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = 1 << (PRECISION_BITS - 1);
  for (int j = 0; j < num; ++j) {
    const int r = first + j;
    if ((unsigned)r >= (unsigned)R) continue;
    const int w = k[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t v = *(const uint32_t*)(inter + (c * a.capv + r) * IST + 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[c][i] += (int)((v >> (8 * i)) & 255u) * w;
    }
  }
  int rgb[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) rgb[c][i] = clamp255(acc[c][i] >> PRECISION_BITS);
  const int x0 = ox0 + 4 * q;
  T* o = out + f * a.sn + (long)(oy0 + ty) * a.sy + (long)x0 * a.sx;
  store_rgb4(o, rgb, x0, a.ow, a.sc, a.sx);
}

double filter_support(int filter) { return filter == SF_RESIZE_BICUBIC ? 2.0 : 1.0; }

// the most input pixels a run of `tile` outputs reaches: xmin(first) > c_first - support - 1/2 and xend(last) <= c_last +
// support + 1/2 (resize_reference.coefficients), so the extent is below (tile - 1) scale + 2 support + 1; two more for the
// rounding of this expression
int tile_extent(int in_size, int out_size, int filter, int tile) {
  const double scale = (double)in_size / out_size, support = filter_support(filter) * (scale > 1.0 ? scale : 1.0);
  const double e = (tile - 1) * scale + 2 * support;
  return e + 3 < in_size ? (int)e + 3 : in_size;
}

}  // namespace

extern "C" int sf_resize_kernel_size(int in_size, int out_size, int filter) {
  const char* who = "sf_resize_kernel_size";
  if (filter < SF_RESIZE_BILINEAR || filter > SF_RESIZE_BICUBIC) {
    sf_set_error("%s: unknown filter %d", who, filter);
    return 0;
  }
  if (in_size < 1 || out_size < 1) {
    sf_set_error("%s: sizes %d -> %d (both >= 1)", who, in_size, out_size);
    return 0;
  }
  const double scale = (double)in_size / out_size, support = filter_support(filter) * (scale > 1.0 ? scale : 1.0);
  return (int)ceil(support) * 2 + 1;
}

extern "C" int sf_resize_frames(const void* frames, int layout, int n, int h, int w, const int32_t* crop, const int32_t* bounds_h, const int32_t* coefs_h,
                                const int32_t* bounds_v, const int32_t* coefs_v, int filter, void* out, int out_layout, int out_dtype, int out_h, int out_w,
                                void* stream) {
  const char* who = "sf_resize_frames";
  SF_CHECK(frames && out && bounds_h && coefs_h && bounds_v && coefs_v, "%s: null buffer", who);
  SF_CHECK(layout >= SF_JPEG_HWC && layout <= SF_JPEG_CHW && out_layout >= SF_JPEG_HWC && out_layout <= SF_JPEG_CHW, "%s: unknown layout %d -> %d", who,
           layout, out_layout);
  SF_CHECK(out_dtype >= SF_JPEG_U8 && out_dtype <= SF_JPEG_BF16, "%s: unknown dtype %d", who, out_dtype);
  SF_CHECK(filter >= SF_RESIZE_BILINEAR && filter <= SF_RESIZE_BICUBIC, "%s: unknown filter %d", who, filter);
  SF_CHECK(n > 0 && n <= 65535, "%s: n=%d frames (1..65535)", who, n);
  SF_CHECK(h > 0 && w > 0 && h <= 65535 && w <= 65535, "%s: frame %dx%d (1..65535)", who, h, w);
  SF_CHECK(out_h > 0 && out_w > 0 && out_h <= 65535 && out_w <= 65535, "%s: output %dx%d (1..65535)", who, out_h, out_w);
  ResizeArgs a;
  a.top = crop ? crop[0] : 0, a.left = crop ? crop[1] : 0, a.ch = crop ? crop[2] : h, a.cw = crop ? crop[3] : w;
  SF_CHECK(a.top >= 0 && a.left >= 0 && a.ch >= 1 && a.cw >= 1 && a.ch <= h - a.top && a.cw <= w - a.left,
           "%s: crop (top %d, left %d, %dx%d) does not lie inside a %dx%d frame", who, a.top, a.left, a.ch, a.cw, h, w);
  SF_CHECK(a.ch <= SF_RESIZE_MAX_RATIO * out_h && a.cw <= SF_RESIZE_MAX_RATIO * out_w,
           "%s: %dx%d -> %dx%d reduces by more than %dx, the limit per axis", who, a.ch, a.cw, out_h, out_w, SF_RESIZE_MAX_RATIO);
  SF_CHECK((uintptr_t)frames % 4 == 0 && (uintptr_t)out % 16 == 0, "%s: frames must be 4-byte, out 16-byte aligned", who);
  SF_CHECK(((uintptr_t)bounds_h | (uintptr_t)coefs_h | (uintptr_t)bounds_v | (uintptr_t)coefs_v) % 4 == 0, "%s: the tables must be 4-byte aligned", who);
  a.in = (const uint8_t*)frames;
  a.in_bytes = 3L * n * h * w;
  const FrameStrides in = frame_strides(layout, n, h, w), to = frame_strides(out_layout, n, out_h, out_w);
  a.in_sn = in.sn, a.in_sc = in.sc, a.in_sy = in.sy, a.in_sx = in.sx, a.sn = to.sn, a.sc = to.sc, a.sy = to.sy, a.sx = to.sx;
  a.bh = bounds_h, a.kh = coefs_h, a.bv = bounds_v, a.kv = coefs_v;
  a.ksh = sf_resize_kernel_size(a.cw, out_w, filter), a.ksv = sf_resize_kernel_size(a.ch, out_h, filter);
  a.oh = out_h, a.ow = out_w;
  a.caph = tile_extent(a.cw, out_w, filter, TW), a.capv = tile_extent(a.ch, out_h, filter, TH);
  a.nseg = layout == SF_JPEG_HWC ? 1 : 3;
  a.seg_stride = (a.caph * (a.nseg == 1 ? 3 : 1) + 3 + 3) & ~3;              // the run and up to three bytes in front of it, in whole dwords
  a.rb = STAGE_BYTES / (a.nseg * a.seg_stride);
  a.rb = a.rb < 1 ? 1 : (a.rb > 32 ? 32 : a.rb);
  if (a.rb > a.capv) a.rb = a.capv;
  const size_t lds = (size_t)(2 * TW + TW * a.ksh + 2 * TH + TH * a.ksv) * 4 + (size_t)((3 * a.capv * IST + 3) & ~3) + (size_t)a.rb * a.nseg * a.seg_stride;
  SF_CHECK(lds <= 65536, "%s: %zu bytes of LDS for %dx%d -> %dx%d", who, lds, a.ch, a.cw, out_h, out_w);
  const dim3 grid((unsigned)((out_w + TW - 1) / TW), (unsigned)((out_h + TH - 1) / TH), (unsigned)n);
  hipStream_t s = (hipStream_t)stream;
  return pixel_dispatch(out_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return sf_launch<&resize_kernel<T>>(who, grid, dim3(256), lds, s, a, (T*)out);
  });
}
