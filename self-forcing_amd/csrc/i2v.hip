// Row-wise kernels of the generator's i2v model type for gfx950 (MI355X): what the t2v path has no kernel for.
//   patchify_i2v     the 36-channel patch gather: cat([x, y], channel) of causal_model.py:771-775 read from its two
//                    sources, written as the K = 192 operand of the patch GEMM (144 columns + zero padding)
//   layernorm_rows   nn.LayerNorm over any width that is a multiple of 8 (img_emb.proj.0 normalises clip_dim = 1280,
//                    which the one-wave-per-row kernels of elementwise.hip, built for multiples of 512, cannot hold)
//   assemble_y       a chunk of the conditioning tensor y: 4 mask channels + the VAE encoder's 16 fp32 latent channels
//                    (+ the reference-pose map) -> bf16 [20, f, h, w] through a channel and a frame stride
// The first two are HBM-bound; they run once per pass (the gather) and once per prompt (the norm).  assemble_y runs once
// per chunk on a few hundred KB (scalar fp32 reads, a strided gather of the map): not measured against any bound.
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
// The mean is kept as two floats, mean + mean_lo (the fma gives the division's remainder exactly): rounded to one float
// it is off by up to 2^-25 |mean|, which for a row far from zero (N(1000, 4^2): 3e-5 against deviations of 4) moved
// x - mean by 1e-5 relative, 20-60 times the rest of the kernel's error wherever xhat w + b cancels.
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
  const float total = wave_sum(s);
  const float mean = total / (float)C;
  const float mean_lo = fmaf(-mean, (float)C, total) / (float)C;
  float q = 0.f;
  for (int c = lane * 8; c < C; c += 512) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(xr + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = ((float)t[j] - mean) - mean_lo;
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
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)((((float)t[j] - mean) - mean_lo) * rstd * (float)wv[j] + (float)bv[j]);
    *reinterpret_cast<bf16x8*>(orow + c) = o;
  }
}

// One thread per 16-byte group of one H x W plane of y.  blockIdx.y = c * f + t names the plane; its groups are counted
// from the 16-byte boundary at or below the plane's first element (`off` elements in front of it), so every whole group
// is one aligned bf16x8 store whatever the strides are; the groups that hang over either end of the plane store their
// elements one by one.  c < mask_ch: the mask (1 in the clip's frame 0); else bf16(latent[t][c - mask_ch]).  With a map
// ([h*w][C] channels-last bf16): bf16(float(that) + float(map)) -- two roundings, as `y.to(bf16) + map` in torch.
__global__ __launch_bounds__(256) void assemble_y_kernel(const float* __restrict__ latent, const bf16_t* __restrict__ map, bf16_t* __restrict__ y,
                                                         int f, int mask_ch, int C, int hw, long y_cstride, long y_fstride, int first_is_frame0) {
  const int c = blockIdx.y / f, t = blockIdx.y - c * f;
  bf16_t* plane = y + c * y_cstride + t * y_fstride;
  const int off = (int)(((uintptr_t)plane >> 1) & 7);
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int p0 = g * 8 - off;                     // first element of this group, relative to the plane
  if (p0 >= hw) return;
  const float* src = c < mask_ch ? nullptr : latent + ((long)t * (C - mask_ch) + (c - mask_ch)) * hw;
  const float mask = (first_is_frame0 && t == 0) ? 1.f : 0.f;
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int p = p0 + j;
    bf16_t v = (bf16_t)0.f;
    if (p >= 0 && p < hw) {
      v = (bf16_t)(src ? src[p] : mask);
      if (map) v = (bf16_t)((float)v + (float)map[(long)p * C + c]);
    }
    o[j] = v;
  }
  if (p0 >= 0 && p0 + 8 <= hw) {
    *reinterpret_cast<bf16x8*>(plane + p0) = o;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (p0 + j >= 0 && p0 + j < hw) plane[p0 + j] = o[j];
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
  return sf_launch<&patchify_i2v_kernel>("sf_patchify_i2v", dim3(gx), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)y, (bf16_t*)cols,
                                         total, F, x_channels, y_channels, pad_channels, H, W, (long)y_bstride, (long)y_cstride, (long)y_fstride);
}

extern "C" int sf_layernorm_rows(const void* x, const void* weight, const void* bias, void* out, int M, int C, float eps, void* stream) {
  SF_CHECK(x && weight && bias && out, "sf_layernorm_rows: null tensor");
  SF_CHECK(M > 0 && C > 0 && C % 8 == 0, "sf_layernorm_rows: unsupported shape M=%d C=%d (C must be a multiple of 8)", M, C);
  SF_CHECK(((uintptr_t)x | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)out) % 16 == 0, "sf_layernorm_rows: misaligned tensor");
  return sf_launch<&layernorm_rows_kernel>("sf_layernorm_rows", dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                                           (const bf16_t*)weight, (const bf16_t*)bias, (bf16_t*)out, M, C, eps);
}

extern "C" int sf_i2v_assemble_y(const void* latent, const void* ref_map, void* y, int frames, int mask_channels, int latent_channels, int h, int w,
                                 int64_t y_cstride, int64_t y_fstride, int first_is_frame0, void* stream) {
  SF_CHECK(latent && y, "sf_i2v_assemble_y: null tensor");
  SF_CHECK(frames > 0 && mask_channels > 0 && latent_channels > 0 && h > 0 && w > 0,
           "sf_i2v_assemble_y: non-positive size (frames=%d mask_channels=%d latent_channels=%d h=%d w=%d)", frames, mask_channels, latent_channels, h, w);
  const int64_t hw = (int64_t)h * w;
  const int64_t planes = (int64_t)(mask_channels + latent_channels) * frames;
  SF_CHECK(hw <= (int64_t)1 << 30 && planes <= 65535, "sf_i2v_assemble_y: %lld planes of %lld elements exceed the grid", (long long)planes, (long long)hw);
  SF_CHECK(y_cstride >= hw && y_fstride >= hw, "sf_i2v_assemble_y: y's strides (channel %lld, frame %lld) are smaller than a plane of %lld",
           (long long)y_cstride, (long long)y_fstride, (long long)hw);
  SF_CHECK((uintptr_t)latent % 4 == 0 && (uintptr_t)y % 2 == 0 && (!ref_map || (uintptr_t)ref_map % 2 == 0), "sf_i2v_assemble_y: misaligned tensor");
  const unsigned groups = (unsigned)((hw + 7 + 7) / 8);   // a plane that starts inside a group spills into one more
  return sf_launch<&assemble_y_kernel>("sf_i2v_assemble_y", dim3((groups + 255) / 256, (unsigned)planes), dim3(256), 0, (hipStream_t)stream,
                                       (const float*)latent, (const bf16_t*)ref_map, (bf16_t*)y, frames, mask_channels, mask_channels + latent_channels,
                                       (int)hw, (long)y_cstride, (long)y_fstride, first_is_frame0);
}
