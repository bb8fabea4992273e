// Row-wise kernels of the generator's i2v model type for gfx950 (MI355X): what the t2v path has no kernel for.
//   patchify_i2v     the 36-channel patch gather: cat([x, y], channel) of causal_model.py:771-775 read from its two
//                    sources, written as the K = 192 operand of the patch GEMM (144 columns + zero padding)
//   layernorm_rows   nn.LayerNorm over any width that is a multiple of 8 (img_emb.proj.0 normalises clip_dim = 1280,
//                    which the one-wave-per-row kernels of elementwise.hip, built for multiples of 512, cannot hold)
// Both are HBM-bound and run once per pass (the gather) or once per prompt (the norm).
#include "sf_common.h"
#include "../../include/sf_hip.h"

namespace {

// One thread per (token, channel): the 2 x 2 patch of channel c -> columns c * 4 + p * 2 + q of the token's row.
// c < cx reads x [B, F, cx, H, W]; cx <= c < cx + cy reads y [B, cy, F, H, W] through its strides (batch stride 0: one
// image for the whole batch); c >= cx + cy writes the padding zeros.
__global__ __launch_bounds__(256) void patchify_i2v_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y, bf16_t* __restrict__ cols,
                                                           long total, int F, int cx, int cy, int cpad, int H, int W, long y_bstride,
                                                           long y_cstride, long y_fstride) {
  const int h2 = H >> 1, w2 = W >> 1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    // i enumerates (bf, hh, ww, c) with c < cpad
    const int c = (int)(i % cpad);
    long r = i / cpad;
    const int ww = (int)(r % w2); r /= w2;
    const int hh = (int)(r % h2);
    const long bf = r / h2;
    bf16x4 o = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    if (c < cx + cy) {
      const bf16_t* s;
      if (c < cx) {
        s = x + ((bf * cx + c) * H + 2 * hh) * (long)W + 2 * ww;
      } else {
        const long b = bf / F, f = bf - b * F;
        s = y + b * y_bstride + (long)(c - cx) * y_cstride + f * y_fstride + (long)(2 * hh) * W + 2 * ww;
      }
      o[0] = s[0]; o[1] = s[1]; o[2] = s[W]; o[3] = s[W + 1];
    }
    *reinterpret_cast<bf16x4*>(cols + ((bf * h2 + hh) * w2 + ww) * (long)(cpad * 4) + c * 4) = o;
  }
}

// One wave per row, any C % 8 == 0: lane l walks the 16-byte chunks l, l + 64, ...  Mean, then the variance about it,
// then the output: three passes over a row that stays in the cache (at most a few KiB).
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ weight,
                                                             const bf16_t* __restrict__ bias, bf16_t* __restrict__ out, int M, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;   // (wave-uniform)
  const bf16_t* xr = x + (long)row * C;
  float s = 0.f;
  for (int c = lane * 8; c < C; c += 512) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(xr + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += (float)t[j];
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane * 8; c < C; c += 512) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(xr + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = (float)t[j] - mean;
      q += d * d;
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
  bf16_t* orow = out + (long)row * C;
  for (int c = lane * 8; c < C; c += 512) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(xr + c);
    const bf16x8 wv = *reinterpret_cast<const bf16x8*>(weight + c);
    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bias + c);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)(((float)t[j] - mean) * rstd * (float)wv[j] + (float)bv[j]);
    *reinterpret_cast<bf16x8*>(orow + c) = o;
  }
}

}  // namespace

extern "C" int sf_patchify_i2v(const void* x, const void* y, void* cols, int B, int F, int x_channels, int y_channels, int pad_channels,
                               int H, int W, int64_t y_bstride, int64_t y_cstride, int64_t y_fstride, void* stream) {
  SF_CHECK(x && y && cols && B > 0 && F > 0 && x_channels > 0 && y_channels > 0, "sf_patchify_i2v: bad arguments");
  SF_CHECK(H % 2 == 0 && W % 2 == 0 && H > 0 && W > 0, "sf_patchify_i2v: latent H=%d W=%d must be even (patch 2x2)", H, W);
  SF_CHECK(pad_channels >= x_channels + y_channels, "sf_patchify_i2v: %d + %d channels do not fit the %d of a cols row", x_channels, y_channels,
           pad_channels);
  SF_CHECK(y_bstride >= 0 && y_cstride >= (int64_t)H * W && y_fstride >= (int64_t)H * W, "sf_patchify_i2v: y's frames must be contiguous H x W planes");
  const long total = (long)B * F * (H / 2) * (W / 2) * pad_channels;
  const int gx = (int)min((long)4096, (total + 255) / 256);
  hipLaunchKernelGGL(patchify_i2v_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)y, (bf16_t*)cols, total, F,
                     x_channels, y_channels, pad_channels, H, W, (long)y_bstride, (long)y_cstride, (long)y_fstride);
  SF_HIP_LAUNCH_CHECK("sf_patchify_i2v");
  return 0;
}

extern "C" int sf_layernorm_rows(const void* x, const void* weight, const void* bias, void* out, int M, int C, float eps, void* stream) {
  SF_CHECK(x && weight && bias && out, "sf_layernorm_rows: null tensor");
  SF_CHECK(M > 0 && C > 0 && C % 8 == 0, "sf_layernorm_rows: unsupported shape M=%d C=%d (C must be a multiple of 8)", M, C);
  SF_CHECK(((uintptr_t)x | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)out) % 16 == 0, "sf_layernorm_rows: misaligned tensor");
  hipLaunchKernelGGL(layernorm_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)weight,
                     (const bf16_t*)bias, (bf16_t*)out, M, C, eps);
  SF_HIP_LAUNCH_CHECK("sf_layernorm_rows");
  return 0;
}
