// CLIP image encoder for gfx950: CLIPModel.visual (wan/modules/clip.py:527-542) = bicubic resize + normalisation, then
// the ViT-H/14 vision tower with use_31_block=True (clip.py:279-297).  All matrix products (patch embedding as a GEMM over
// patch rows, to_qkv, proj, mlp.0, mlp.2) go through sf_gemm_bf16 with SF_EPI_BIAS; this file holds what the rollout's
// kernels cannot do for a ViT: the preprocessing, an fp32 residual stream with its fused add + LayerNorm (the reference
// keeps x in fp32 under autocast, clip.py:47-50; a bf16 stream costs 1.7-2.8x the reference's own bf16 error at depth, DESIGN.md
// section 15), attention at head dimension 80, and the erf GELU.  One pass per conditioning image: 330 GFLOP per frame,
// 97 % of it in the GEMMs.
#include <cmath>
#include "sf_host.h"

namespace {

constexpr int CLIP_D = 80;          // head dimension
constexpr int CLIP_KS = 88;         // K row stride in LDS (bf16): 176 B, 16-byte aligned, rows spread over the banks
constexpr int CLIP_MAX_L = 480;     // K [Lp][88] + V^T [80][Lp + 8] in bf16 <= 160 KiB of LDS
constexpr int CLIP_MAX_DIM = 8192;  // one fp32 row in LDS

// ------------------------------------------------------------------------------------------ preprocessing
// cubic convolution weights of F.interpolate(mode='bicubic'): A = -0.75
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.0f, x3 = 2.0f - t, x2 = 1.0f - t;
  w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  w[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

template <typename T>
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const T* __restrict__ frames, bf16_t* __restrict__ rows, long total, int H, int W,
                                                              int S, int patch, int kp, float scale_y, float scale_x) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % kp);
  const long row = idx / kp;
  const int pp = patch * patch;
  if (k >= 3 * pp) {
    rows[idx] = (bf16_t)0.f;
    return;
  }
  const int g = S / patch;
  const int pidx = (int)(row % (g * g)), b = (int)(row / (g * g));
  const int c = k / pp, i = (k - c * pp) / patch, j = k - c * pp - i * patch;
  const int oy = (pidx / g) * patch + i, ox = (pidx % g) * patch + j;
  // align_corners=False: source coordinate of the output pixel's centre; taps clamped to the edge, overshoot kept
  const float sy = scale_y * ((float)oy + 0.5f) - 0.5f, sx = scale_x * ((float)ox + 0.5f) - 0.5f;
  const float fy = floorf(sy), fx = floorf(sx);
  float wy[4], wx[4];
  cubic_weights(sy - fy, wy);
  cubic_weights(sx - fx, wx);
  const int iy = (int)fy, ix = (int)fx;
  const T* src = frames + ((long)b * 3 + c) * H * W;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int y = min(max(iy - 1 + a, 0), H - 1);
    float line = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = min(max(ix - 1 + e, 0), W - 1);
      line += wx[e] * (float)src[(long)y * W + x];
    }
    acc += wy[a] * line;
  }
  const float mean = c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f);
  const float sd = c == 0 ? 0.26862954f : (c == 1 ? 0.26130258f : 0.27577711f);
  rows[idx] = (bf16_t)((acc * 0.5f + 0.5f - mean) / sd);
}

// ------------------------------------------------------------------------------------------ fp32 stream: add + LayerNorm
// Sum over the 256 threads of a block; `red` holds 4 floats.  Every thread must call it.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// mean and 1/sqrt(var + eps) of the row a block holds in LDS (each thread its own columns c4 = tid, tid + 256, ...):
// two passes over LDS, one over memory
__device__ __forceinline__ void row_stats(const f32x4* row, int dim4, float eps, float* red, float& mean, float& rstd) {
  float s = 0.f;
  for (int c = threadIdx.x; c < dim4; c += 256) {
    const f32x4 v = row[c];
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  mean = block_sum(s, red) / (float)(dim4 * 4);
  float q = 0.f;
  for (int c = threadIdx.x; c < dim4; c += 256) {
    const f32x4 v = row[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) q += (v[j] - mean) * (v[j] - mean);
  }
  rstd = 1.0f / sqrtf(block_sum(q, red) / (float)(dim4 * 4) + eps);
}

__device__ __forceinline__ f32x4 affine(f32x4 v, float mean, float rstd, f32x4 w, f32x4 b) {
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean) * rstd * w[j] + b[j];
  return o;
}

__device__ __forceinline__ bf16x4 to_bf16x4(f32x4 v) {
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (bf16_t)v[j];
  return o;
}

// one block per row
__global__ __launch_bounds__(256) void clip_add_layernorm_kernel(float* __restrict__ x32, const bf16_t* __restrict__ y, const float* __restrict__ ln_w,
                                                                 const float* __restrict__ ln_b, bf16_t* __restrict__ xn, int dim, float eps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[4];
  f32x4* row = reinterpret_cast<f32x4*>(smem);
  const int dim4 = dim / 4;
  f32x4* x = reinterpret_cast<f32x4*>(x32 + (long)blockIdx.x * dim);
  const bf16x4* yr = reinterpret_cast<const bf16x4*>(y + (long)blockIdx.x * dim);
  for (int c = threadIdx.x; c < dim4; c += 256) {
    f32x4 v = x[c];
    const bf16x4 t = yr[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += (float)t[j];
    x[c] = v;
    row[c] = v;
  }
  if (ln_w == nullptr) return;
  float mean, rstd;
  row_stats(row, dim4, eps, red, mean, rstd);
  bf16x4* o = reinterpret_cast<bf16x4*>(xn + (long)blockIdx.x * dim);
  for (int c = threadIdx.x; c < dim4; c += 256)
    o[c] = to_bf16x4(affine(row[c], mean, rstd, reinterpret_cast<const f32x4*>(ln_w)[c], reinterpret_cast<const f32x4*>(ln_b)[c]));
}

// one block per token row: cls / patch embedding + position, pre_norm into the stream, norm1 of block 0 into xn
__global__ __launch_bounds__(256) void clip_embed_norm_kernel(const bf16_t* __restrict__ patch_out, const float* __restrict__ cls, const float* __restrict__ pos,
                                                              const float* __restrict__ pre_w, const float* __restrict__ pre_b,
                                                              const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                              float* __restrict__ x32, bf16_t* __restrict__ xn, int P, int dim, float eps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[4];
  f32x4* row = reinterpret_cast<f32x4*>(smem);
  const int dim4 = dim / 4, L = P + 1;
  const int b = blockIdx.x / L, t = blockIdx.x - b * L;
  const f32x4* pr = reinterpret_cast<const f32x4*>(pos + (long)t * dim);
  const bf16x4* er = reinterpret_cast<const bf16x4*>(patch_out + ((long)b * P + (t > 0 ? t - 1 : 0)) * dim);
  for (int c = threadIdx.x; c < dim4; c += 256) {
    f32x4 v;
    if (t == 0) {
      v = reinterpret_cast<const f32x4*>(cls)[c];
    } else {
      const bf16x4 e = er[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)e[j];
    }
    const f32x4 p = pr[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += p[j];
    row[c] = v;
  }
  float mean, rstd;
  row_stats(row, dim4, eps, red, mean, rstd);
  f32x4* x = reinterpret_cast<f32x4*>(x32 + (long)blockIdx.x * dim);
  for (int c = threadIdx.x; c < dim4; c += 256) {
    const f32x4 v = affine(row[c], mean, rstd, reinterpret_cast<const f32x4*>(pre_w)[c], reinterpret_cast<const f32x4*>(pre_b)[c]);
    x[c] = v;
    row[c] = v;
  }
  if (ln_w == nullptr) return;
  row_stats(row, dim4, eps, red, mean, rstd);
  bf16x4* o = reinterpret_cast<bf16x4*>(xn + (long)blockIdx.x * dim);
  for (int c = threadIdx.x; c < dim4; c += 256)
    o[c] = to_bf16x4(affine(row[c], mean, rstd, reinterpret_cast<const f32x4*>(ln_w)[c], reinterpret_cast<const f32x4*>(ln_b)[c]));
}

// ------------------------------------------------------------------------------------------ GELU
// x Phi(x) = x/2 erfc(-x / sqrt 2): erfc keeps the left tail, where 1 + erf cancels
__global__ __launch_bounds__(256) void clip_gelu_kernel(const bf16x8* __restrict__ x, bf16x8* __restrict__ out, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const bf16x8 v = x[i];
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = (float)v[j];
    o[j] = (bf16_t)(0.5f * f * erfcf(-0.70710678118654752f * f));
  }
  out[i] = o;
}

// ------------------------------------------------------------------------------------------ attention, D = 80
// One workgroup per (64 queries, head, image); wave w owns queries 16 w .. 16 w + 15.  K [Lp][88] and V^T [80][Lp + 8] of the
// (image, head) sit in LDS, keys padded to Lp = a multiple of 32 with zeros.  Both products are computed transposed on
// v_mfma_f32_16x16x32_bf16, so that the scores a lane holds are already the fragment of the second product:
//   S^T [key][query] = K . Q^T   lane (g = lane >> 4, r = lane & 15): A = K[16 t + r][8 g + j], B = Q[query r][8 g + j];
//                                result register i = key 16 t + 4 g + i of query r.  d = 80 is two and a half k-steps:
//                                in the third, lane groups 2 and 3 (d 80..95) contribute zero fragments.
//   O^T [d][query]   = V^T . P^T over 32 keys: the lane's B fragment = its own 8 probabilities of score tiles 2 c and 2 c + 1
//                                (keys 32 c + 4 g + i and 32 c + 16 + 4 g + i), its A fragment = V^T[d = 16 u + r] at those
//                                same keys (two 8-byte LDS reads); result register i = d 16 u + 4 g + i of query r.
// The softmax is two passes over the resident K (row maximum, then exponentials and P.V); the scores are recomputed rather
// than kept -- Q.K^T is a fifth of this kernel's matrix work and the kernel 3 % of the encoder's -- so nothing is indexed
// by L.  Keys >= L get P = 0 against V = 0.
__global__ __launch_bounds__(256) void clip_attention_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int L, int H, int Lp, float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);
  const int vts = Lp + 8;
  bf16_t* Vt = Ks + (long)Lp * CLIP_KS;
  const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * 64;
  const long tok = 3L * H * CLIP_D;
  const bf16_t* qb = qkv + (long)b * L * tok + (long)h * CLIP_D;
  const bf16_t* kb = qb + (long)H * CLIP_D;
  const bf16_t* vb = kb + (long)H * CLIP_D;
  bf16x8 zero8;
#pragma unroll
  for (int j = 0; j < 8; ++j) zero8[j] = (bf16_t)0.f;

  for (int i = tid; i < Lp * 10; i += 256) {
    const int row = i / 10, c = i - row * 10;
    bf16x8 kv = zero8, vv = zero8;
    if (row < L) {
      kv = *reinterpret_cast<const bf16x8*>(kb + row * tok + c * 8);
      vv = *reinterpret_cast<const bf16x8*>(vb + row * tok + c * 8);
    }
    *reinterpret_cast<bf16x8*>(Ks + row * CLIP_KS + c * 8) = kv;
#pragma unroll
    for (int j = 0; j < 8; ++j) Vt[(c * 8 + j) * vts + row] = vv[j];
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, r = lane & 15;
  if (q0 + wave * 16 >= L) return;            // a whole wave without queries (after the only barrier)
  const int query = q0 + wave * 16 + r;
  const bf16_t* qr = qb + (long)min(query, L - 1) * tok + g * 8;
  const bf16x8 qf0 = *reinterpret_cast<const bf16x8*>(qr), qf1 = *reinterpret_cast<const bf16x8*>(qr + 32);
  const bf16x8 qf2 = g < 2 ? *reinterpret_cast<const bf16x8*>(qr + 64) : zero8;

  auto scores = [&](int tile) {
    const bf16_t* kr = Ks + (tile * 16 + r) * CLIP_KS + g * 8;
    const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(kr), a1 = *reinterpret_cast<const bf16x8*>(kr + 32);
    const bf16x8 a2 = g < 2 ? *reinterpret_cast<const bf16x8*>(kr + 64) : zero8;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qf0, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qf1, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, qf2, s, 0, 0, 0);
    return s;
  };

  float m = -INFINITY;
  for (int t = 0; t < Lp / 16; ++t) {
    const f32x4 s = scores(t);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (t * 16 + 4 * g + i < L) m = fmaxf(m, s[i]);
  }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));

  float sum = 0.f;
  f32x4 o[5];
#pragma unroll
  for (int u = 0; u < 5; ++u) o[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < Lp / 32; ++c) {
    const f32x4 s0 = scores(2 * c), s1 = scores(2 * c + 1);
    bf16x8 pf;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = c * 32 + 4 * g + i;
      const float p0 = key < L ? __builtin_amdgcn_exp2f((s0[i] - m) * scale_log2e) : 0.f;
      const float p1 = key + 16 < L ? __builtin_amdgcn_exp2f((s1[i] - m) * scale_log2e) : 0.f;
      sum += p0 + p1;
      pf[i] = (bf16_t)p0;
      pf[4 + i] = (bf16_t)p1;
    }
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const bf16_t* vr = Vt + (u * 16 + r) * vts + c * 32 + 4 * g;
      const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr), hi = *reinterpret_cast<const bf16x4*>(vr + 16);
      bf16x8 vf;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        vf[i] = lo[i];
        vf[4 + i] = hi[i];
      }
      o[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[u], 0, 0, 0);
    }
  }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  if (query >= L) return;
  const float inv = 1.0f / sum;
  bf16_t* orow = out + ((long)b * L + query) * H * CLIP_D + h * CLIP_D + 4 * g;
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    bf16x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (bf16_t)(o[u][i] * inv);
    *reinterpret_cast<bf16x4*>(orow + u * 16) = w;
  }
}

// ------------------------------------------------------------------------------------------ sequencer
struct Work {
  char *rows, *patch, *xn, *qkv, *ao, *y, *h;
  size_t total;
};

Work carve(const sf_clip_model* m, void* ws, int n) {
  Work w;
  const int g = m->image_size / m->patch;
  const size_t P = (size_t)g * g, M = (size_t)n * (P + 1), D = m->dim, kp = (3 * (size_t)m->patch * m->patch + 63) / 64 * 64;
  Carve c(ws);
  w.rows = c.take((size_t)n * P * kp * 2);
  w.patch = c.take((size_t)n * P * D * 2);
  w.xn = c.take(M * D * 2);
  w.qkv = c.take(M * 3 * D * 2);
  w.ao = c.take(M * D * 2);
  w.y = c.take(M * D * 2);
  w.h = c.take(M * (size_t)m->mlp_dim * 2);
  w.total = c.off;
  return w;
}

int check_model(const sf_clip_model* m, int n) {
  SF_CHECK(m != nullptr, "sf_clip: null model");
  SF_CHECK(n > 0, "sf_clip: n=%d frames", n);
  SF_CHECK(m->patch > 0 && m->image_size > 0 && m->image_size % m->patch == 0, "sf_clip: image_size=%d must be a multiple of patch=%d", m->image_size, m->patch);
  SF_CHECK(m->dim > 0 && m->dim % 64 == 0 && m->dim <= CLIP_MAX_DIM, "sf_clip: dim=%d must be a multiple of 64, at most %d", m->dim, CLIP_MAX_DIM);
  SF_CHECK(m->heads > 0 && m->dim == m->heads * CLIP_D, "sf_clip: head dimension must be 80 (dim=%d heads=%d)", m->dim, m->heads);
  SF_CHECK(m->mlp_dim > 0 && m->mlp_dim % 64 == 0, "sf_clip: mlp_dim=%d must be a multiple of 64", m->mlp_dim);
  const long g = m->image_size / m->patch, L = g * g + 1;
  SF_CHECK(L <= CLIP_MAX_L, "sf_clip: %ld tokens per image, the attention kernel holds at most %d", L, CLIP_MAX_L);
  SF_CHECK((long)n * L * m->mlp_dim < (1L << 31), "sf_clip: n=%d frames exceed the 2^31-element activations", n);
  SF_CHECK(m->layers_built >= 0 && (m->layers_built == 0 || m->layers_host), "sf_clip: null tensor (layers_host)");
  SF_CHECK(m->patch_w && m->cls && m->pos && m->pre_norm_w && m->pre_norm_b, "sf_clip: null tensor in the embedding");
  for (int l = 0; l < m->layers_built; ++l) {
    const sf_clip_layer& y = m->layers_host[l];
    SF_CHECK(y.norm1_w && y.norm1_b && y.qkv_w && y.qkv_b && y.proj_w && y.proj_b && y.norm2_w && y.norm2_b && y.fc1_w && y.fc1_b && y.fc2_w && y.fc2_b,
             "sf_clip: null tensor in block %d", l);
  }
  return 0;
}

// out [M, N] = a [M, K] . w [N, K]^T + bias on 128 x 128 tiles whatever M is: the automatic choice moves to the ping-pong
// structure at M >= 1024, and a frame must come out the same alone and in a batch
int linear(const void* a, const void* w, const void* bias, void* out, int M, int N, int K, void* stream) {
  Gemm gm(a, K, w, K, out, N, M, N, K);
  gm.bias(bias);
  gm.g.structure = SF_GEMM_T128;
  return gm.bf16(stream);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sf_clip_preprocess(const void* frames, int dtype, int n, int H, int W, int image_size, int patch, int kp, void* rows, void* stream) {
  SF_CHECK(frames && rows, "sf_clip_preprocess: null tensor");
  SF_CHECK(dtype == SF_CLIP_F32 || dtype == SF_CLIP_BF16, "sf_clip_preprocess: unknown dtype %d", dtype);
  SF_CHECK(n > 0 && H > 0 && W > 0, "sf_clip_preprocess: n=%d frames of %d x %d", n, H, W);
  SF_CHECK(patch > 0 && image_size > 0 && image_size % patch == 0, "sf_clip_preprocess: image_size=%d must be a multiple of patch=%d", image_size, patch);
  SF_CHECK(kp >= 3 * patch * patch, "sf_clip_preprocess: kp=%d is less than 3 x patch x patch = %d", kp, 3 * patch * patch);
  const long total = (long)n * image_size * image_size / (patch * patch) * kp;
  SF_CHECK(total < (1L << 40) && (total + 255) / 256 < (1L << 31), "sf_clip_preprocess: n=%d frames are too many for one launch", n);
  const float sy = (float)H / (float)image_size, sx = (float)W / (float)image_size;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (dtype == SF_CLIP_F32)
    return sf_launch<&clip_preprocess_kernel<float>>("sf_clip_preprocess", grid, block, 0, (hipStream_t)stream, (const float*)frames, (bf16_t*)rows, total, H,
                                                     W, image_size, patch, kp, sy, sx);
  return sf_launch<&clip_preprocess_kernel<bf16_t>>("sf_clip_preprocess", grid, block, 0, (hipStream_t)stream, (const bf16_t*)frames, (bf16_t*)rows, total, H,
                                                    W, image_size, patch, kp, sy, sx);
}

extern "C" int sf_clip_embed_norm(const void* patch_out, const float* cls, const float* pos, const float* pre_w, const float* pre_b, const float* ln_w,
                                  const float* ln_b, float* x32, void* xn, int n, int P, int dim, float eps, void* stream) {
  SF_CHECK(patch_out && cls && pos && pre_w && pre_b && x32, "sf_clip_embed_norm: null tensor");
  SF_CHECK(ln_w == nullptr || (ln_b && xn), "sf_clip_embed_norm: ln_w needs ln_b and xn");
  SF_CHECK(n > 0 && P > 0 && dim > 0 && dim % 4 == 0 && dim <= CLIP_MAX_DIM, "sf_clip_embed_norm: n=%d P=%d dim=%d (dim a multiple of 4, at most %d)", n, P, dim, CLIP_MAX_DIM);
  SF_CHECK((long)n * (P + 1) < (1L << 31), "sf_clip_embed_norm: too many rows");
  SF_CHECK(aligned16(cls) && aligned16(pos) && aligned16(pre_w) && aligned16(pre_b) && aligned16(ln_w) && aligned16(ln_b) && aligned16(x32) &&
               ((uintptr_t)patch_out & 7) == 0 && ((uintptr_t)xn & 7) == 0, "sf_clip_embed_norm: misaligned tensor");
  return sf_launch<&clip_embed_norm_kernel>("sf_clip_embed_norm", dim3(n * (P + 1)), dim3(256), (size_t)dim * 4, (hipStream_t)stream, (const bf16_t*)patch_out,
                                            cls, pos, pre_w, pre_b, ln_w, ln_b, x32, (bf16_t*)xn, P, dim, eps);
}

extern "C" int sf_clip_add_layernorm(float* x32, const void* y, const float* ln_w, const float* ln_b, void* xn, int rows, int dim, float eps, void* stream) {
  SF_CHECK(x32 && y, "sf_clip_add_layernorm: null tensor");
  SF_CHECK(ln_w == nullptr || (ln_b && xn), "sf_clip_add_layernorm: ln_w needs ln_b and xn");
  SF_CHECK(rows > 0 && dim > 0 && dim % 4 == 0 && dim <= CLIP_MAX_DIM, "sf_clip_add_layernorm: rows=%d dim=%d (dim a multiple of 4, at most %d)", rows, dim, CLIP_MAX_DIM);
  SF_CHECK(aligned16(x32) && aligned16(ln_w) && aligned16(ln_b) && ((uintptr_t)y & 7) == 0 && ((uintptr_t)xn & 7) == 0, "sf_clip_add_layernorm: misaligned tensor");
  return sf_launch<&clip_add_layernorm_kernel>("sf_clip_add_layernorm", dim3(rows), dim3(256), (size_t)dim * 4, (hipStream_t)stream, x32, (const bf16_t*)y,
                                               ln_w, ln_b, (bf16_t*)xn, dim, eps);
}

extern "C" int sf_clip_attention(const void* qkv, void* out, int n, int L, int H, void* stream) {
  SF_CHECK(qkv && out, "sf_clip_attention: null tensor");
  SF_CHECK(n > 0 && n <= 65535 && H > 0 && H <= 65535, "sf_clip_attention: n=%d images, H=%d heads", n, H);
  SF_CHECK(L >= 1 && L <= CLIP_MAX_L, "sf_clip_attention: L=%d, K and V of one head must fit in LDS (1 <= L <= %d)", L, CLIP_MAX_L);
  SF_CHECK(aligned16(qkv) && ((uintptr_t)out & 7) == 0, "sf_clip_attention: misaligned tensor");
  SF_CHECK((long)n * L * 3 * H * CLIP_D < (1L << 40), "sf_clip_attention: tensor too large");
  const int Lp = (L + 31) & ~31;
  const int lds = (Lp * CLIP_KS + CLIP_D * (Lp + 8)) * 2;
  constexpr int max_lp = (CLIP_MAX_L + 31) & ~31, lds_cap = (max_lp * CLIP_KS + CLIP_D * (max_lp + 8)) * 2;   // the kernel's cap: lds at CLIP_MAX_L
  return sf_launch<&clip_attention_kernel, lds_cap>("sf_clip_attention", dim3((L + 63) / 64, H, n), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)qkv,
                                                    (bf16_t*)out, L, H, Lp, 1.4426950408889634f / sqrtf((float)CLIP_D));
}

extern "C" int sf_clip_gelu(const void* x, void* out, int64_t count, void* stream) {
  SF_CHECK(x && out && count > 0 && count % 8 == 0, "sf_clip_gelu: count=%lld must be a positive multiple of 8", (long long)count);
  SF_CHECK(aligned16(x) && aligned16(out), "sf_clip_gelu: misaligned tensor");
  const long n8 = count / 8;
  SF_CHECK((n8 + 255) / 256 < (1L << 31), "sf_clip_gelu: count=%lld is too large for one launch", (long long)count);
  return sf_launch<&clip_gelu_kernel>("sf_clip_gelu", dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16x8*)x, (bf16x8*)out,
                                      n8);
}

extern "C" size_t sf_clip_workspace_bytes(const sf_clip_model* m, int n) {
  if (check_model(m, n) != 0) return 0;
  return carve(m, nullptr, n).total;
}

extern "C" int sf_clip_encode(const sf_clip_model* m, const void* frames, int dtype, int n, int H, int W, float* out, void* workspace,
                              size_t workspace_bytes, void* stream) {
  SF_TRY(check_model(m, n));
  SF_CHECK(frames && out, "sf_clip_encode: null tensor");
  SF_CHECK(dtype == SF_CLIP_F32 || dtype == SF_CLIP_BF16, "sf_clip_encode: unknown dtype %d", dtype);
  SF_CHECK(H > 0 && W > 0, "sf_clip_encode: frames of %d x %d", H, W);
  const Work w = carve(m, workspace, n);
  SF_CHECK(workspace && workspace_bytes >= w.total, "sf_clip_encode: workspace too small (%zu < %zu)", workspace_bytes, w.total);
  const int g = m->image_size / m->patch, P = g * g, L = P + 1, M = n * L, D = m->dim, F = m->mlp_dim;
  const int kp = (3 * m->patch * m->patch + 63) / 64 * 64;
  const sf_clip_layer* ly = m->layers_host;
  const int nl = m->layers_built;

  SF_TRY(sf_clip_preprocess(frames, dtype, n, H, W, m->image_size, m->patch, kp, w.rows, stream));
  SF_TRY(linear(w.rows, m->patch_w, nullptr, w.patch, n * P, D, kp, stream));        // patch_embedding has no bias (pre_norm)
  SF_TRY(sf_clip_embed_norm(w.patch, m->cls, m->pos, m->pre_norm_w, m->pre_norm_b, nl ? ly[0].norm1_w : nullptr, nl ? ly[0].norm1_b : nullptr,
                            out, w.xn, n, P, D, m->eps, stream));
  for (int l = 0; l < nl; ++l) {
    // x = x + attn(norm1(x))   (clip.py:151)
    SF_TRY(linear(w.xn, ly[l].qkv_w, ly[l].qkv_b, w.qkv, M, 3 * D, D, stream));
    SF_TRY(sf_clip_attention(w.qkv, w.ao, n, L, m->heads, stream));
    SF_TRY(linear(w.ao, ly[l].proj_w, ly[l].proj_b, w.y, M, D, D, stream));
    SF_TRY(sf_clip_add_layernorm(out, w.y, ly[l].norm2_w, ly[l].norm2_b, w.xn, M, D, m->eps, stream));
    // x = x + mlp(norm2(x))    (clip.py:152); the add carries norm1 of the next block, the last one adds only
    SF_TRY(linear(w.xn, ly[l].fc1_w, ly[l].fc1_b, w.h, M, F, D, stream));
    SF_TRY(sf_clip_gelu(w.h, w.h, (int64_t)M * F, stream));
    SF_TRY(linear(w.h, ly[l].fc2_w, ly[l].fc2_b, w.y, M, D, F, stream));
    const bool last = l + 1 == nl;
    SF_TRY(sf_clip_add_layernorm(out, w.y, last ? nullptr : ly[l + 1].norm1_w, last ? nullptr : ly[l + 1].norm1_b, w.xn, M, D, m->eps, stream));
  }
  return 0;
}
