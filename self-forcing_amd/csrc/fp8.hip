// FP8 (OCP e4m3fn) pieces of the opt-in FP8 linear layers for gfx950: the dynamic per-tensor activation quantiser and
// the small-M linear layer on e4m3 weights.  The GEMM itself is gemm_bf16.hip's structures instantiated for e4m3
// (sf_gemm_fp8).
//
// Replaces the reference's optional `quantize_(transformer, Float8DynamicActivationFloat8WeightConfig(
// granularity=PerTensor()))` (demo.py:277-283; README: "using FP8 Linear layers").  torchao's exact rounding is not
// reproduced; the recipe is this project's definition, pinned by the tests:
//   scale   s = max(amax(|x|) as fp32, 1e-12) / 448       over one SEGMENT of rows (the rows of one generator pass)
//   bytes   q = e4m3fn_rne(clamp(x.float() / s, -448, 448))  == torch's (x.float() / s).clamp(-448, 448).to(float8_e4m3fn)
// The division is a true fp32 division (no fast-math flags for this file: the Makefile's defaults), and the
// conversion is v_cvt_pk_fp8_f32 (round to nearest even; the clamp keeps it off the saturation path).
#include "sf_common.h"
#include "../../include/sf_hip.h"

namespace {

constexpr int QT = 256;                       // threads per workgroup of the two quantiser passes
constexpr int PARTS = SF_FP8_AMAX_PARTS;      // partial maxima per segment (scratch slots behind the scales)

// e4m3fn byte -> fp32 (exact).  The quantiser never produces the NaN codes 0x7f / 0xff.
__device__ __forceinline__ float e4m3_to_f32(uint32_t b) {
  const uint32_t e = (b >> 3) & 15u, mnt = b & 7u;
  const float v = e ? __uint_as_float(((e + 120u) << 23) | (mnt << 20)) : (float)mnt * 0.001953125f;   // subnormal: mnt x 2^-9
  return (b & 0x80u) ? -v : v;
}

// four fp32 values (already divided by the scale) -> four e4m3 bytes, clamped to +-448
__device__ __forceinline__ uint32_t pack4_e4m3(float a, float b, float c, float d) {
  const auto cl = [](float v) { return fminf(fmaxf(v, -448.f), 448.f); };
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(a), cl(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(c), cl(d), w, true);
  return (uint32_t)w;
}

__device__ __forceinline__ float block_max(float v, float* red) {   // all threads of a QT-thread workgroup; result in every thread
  v = wave_max(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < QT / 64; ++i) r = fmaxf(r, red[i]);
  return r;
}

// Pass 1: workgroup (part, seg) reduces a strided share of its segment's 8-element chunks to one partial maximum of |x|.
// Every slot [seg][part < parts] is written (plain stores, no atomics): the result does not depend on the order.
__global__ __launch_bounds__(QT) void fp8_amax_kernel(const bf16_t* __restrict__ x, int ldx, int M, int K, int rps, int parts,
                                                      float* __restrict__ partial) {
  __shared__ float red[QT / 64];
  const int seg = blockIdx.y, part = blockIdx.x;
  const int r0 = seg * rps, rows = min(rps, M - r0), kc = K / 8;
  const long n = (long)rows * kc;
  float m = 0.f;
  for (long i = (long)part * QT + threadIdx.x; i < n; i += (long)parts * QT) {
    const int row = (int)(i / kc), c = (int)(i - (long)row * kc);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + (long)(r0 + row) * ldx + c * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf((float)v[j]));
  }
  m = block_max(m, red);
  if (threadIdx.x == 0) partial[seg * PARTS + part] = m;
}

// Pass 2: every wave folds its segment's partial maxima into the scale (at most 16 L2 loads per lane), workgroup
// (0, seg) stores it, and the workgroup writes e4m3 bytes for its share of the segment's chunks.
__global__ __launch_bounds__(QT) void fp8_quantize_kernel(const bf16_t* __restrict__ x, int ldx, int M, int K, int rps, int parts,
                                                          const float* __restrict__ partial, uint8_t* __restrict__ q,
                                                          float* __restrict__ scale_out) {
  const int seg = blockIdx.y, part = blockIdx.x, lane = threadIdx.x & 63;
  float amax = 0.f;
  for (int i = lane; i < parts; i += 64) amax = fmaxf(amax, partial[seg * PARTS + i]);
  amax = wave_max(amax);
  const float s = fmaxf(amax, 1e-12f) / 448.f;
  if (part == 0 && threadIdx.x == 0) scale_out[seg] = s;
  const int r0 = seg * rps, rows = min(rps, M - r0), kc = K / 8;
  const long n = (long)rows * kc;
  for (long i = (long)part * QT + threadIdx.x; i < n; i += (long)parts * QT) {
    const int row = (int)(i / kc), c = (int)(i - (long)row * kc);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + (long)(r0 + row) * ldx + c * 8);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j] / s;
    const u32x2 o = {pack4_e4m3(f[0], f[1], f[2], f[3]), pack4_e4m3(f[4], f[5], f[6], f[7])};
    *reinterpret_cast<u32x2*>(q + (long)(r0 + row) * K + c * 8) = o;
  }
}

// ------------------------------------------------------------------------------------------
// Small-M linear on e4m3 weights (M <= 32): out = act_out(acc * (sa[seg(m)] * w_scale[n]) + bias[n]) with acc the fp32
// sum of e4m3(act_in(x) / sa) x w_q.  Bandwidth bound on the weights, which are half the bytes of the bf16 form.  Every
// workgroup first recomputes the per-segment activation amax itself (x is at most 32 x K and sits in L2), so the whole
// layer is one launch; then the quantised rows, as exact bf16 values, are staged 8 at a time in LDS and every wave
// streams SLF_NPW weight rows against them.
constexpr int SLF_THREADS = 256;
constexpr int SLF_NPW = 4;        // output columns per wave
constexpr int SLF_MB = 8;         // activation rows per LDS pass

__device__ __forceinline__ float act_f(float v, int act) { return act == 1 ? silu_f(v) : (act == 2 ? gelu_tanh_f(v) : v); }

__global__ __launch_bounds__(SLF_THREADS) void small_linear_fp8_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ w,
                                                                       const float* __restrict__ w_scale, const bf16_t* __restrict__ bias,
                                                                       bf16_t* __restrict__ out, int M, int N, int K, int rps,
                                                                       int act_in, int act_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rowmax = reinterpret_cast<float*>(smem);                 // [32]
  float* sa = rowmax + 32;                                        // [32]: the scale of row m's segment
  bf16_t* xs = reinterpret_cast<bf16_t*>(sa + 32);                // [SLF_MB][K]: e4m3 values of the rows (exact in bf16)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // 1. |act_in(x)| maxima per row (the activation rounded to bf16 first, as the bf16 kernel stages it)
  for (int m = wave; m < M; m += SLF_THREADS / 64) {
    float mx = 0.f;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, fabsf((float)(bf16_t)act_f((float)x[(long)m * K + k], act_in)));
    mx = wave_max(mx);
    if (lane == 0) rowmax[m] = mx;
  }
  __syncthreads();
  if (tid < M) {
    const int s0 = (tid / rps) * rps, s1 = min(s0 + rps, M);
    float mx = 0.f;
    for (int m = s0; m < s1; ++m) mx = fmaxf(mx, rowmax[m]);
    sa[tid] = fmaxf(mx, 1e-12f) / 448.f;
  }
  __syncthreads();
  const int n0 = (blockIdx.x * (SLF_THREADS / 64) + wave) * SLF_NPW;
  float ws[SLF_NPW];
#pragma unroll
  for (int c = 0; c < SLF_NPW; ++c) ws[c] = w_scale[min(n0 + c, N - 1)];
  for (int m0 = 0; m0 < M; m0 += SLF_MB) {
    const int mc = min(SLF_MB, M - m0);
    // 2. quantise rows m0 .. m0 + mc into LDS
    for (int i = tid; i < mc * K; i += SLF_THREADS) {
      const int m = i / K, k = i - m * K;
      const float v = (float)(bf16_t)act_f((float)x[(long)(m0 + m) * K + k], act_in);
      const int b = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(v / sa[m0 + m], -448.f), 448.f), 0.f, 0, false);
      xs[i] = (bf16_t)e4m3_to_f32((uint32_t)b & 0xffu);
    }
    __syncthreads();
    // 3. the wave's columns: 8 weight bytes per lane per step, fp32 products (exact) and sums
    float acc[SLF_NPW][SLF_MB];
#pragma unroll
    for (int c = 0; c < SLF_NPW; ++c)
#pragma unroll
      for (int m = 0; m < SLF_MB; ++m) acc[c][m] = 0.f;
    for (int k = lane * 8; k < K; k += 64 * 8) {
      float wf[SLF_NPW][8];
#pragma unroll
      for (int c = 0; c < SLF_NPW; ++c) {
        const u32x2 wv = *reinterpret_cast<const u32x2*>(w + (long)min(n0 + c, N - 1) * K + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) wf[c][j] = e4m3_to_f32((wv[j >> 2] >> (8 * (j & 3))) & 0xffu);
      }
#pragma unroll
      for (int m = 0; m < SLF_MB; ++m) {
        if (m >= mc) break;
        const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xs + m * K + k);
#pragma unroll
        for (int c = 0; c < SLF_NPW; ++c)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[c][m] += (float)xv[j] * wf[c][j];
      }
    }
#pragma unroll
    for (int c = 0; c < SLF_NPW; ++c)
#pragma unroll
      for (int m = 0; m < SLF_MB; ++m) acc[c][m] = wave_sum(acc[c][m]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < SLF_NPW; ++c) {
        const int n = n0 + c;
        if (n >= N) continue;
        const float b = bias ? (float)bias[n] : 0.f;
        for (int m = 0; m < mc; ++m) out[(long)(m0 + m) * N + n] = (bf16_t)act_f(acc[c][m] * (sa[m0 + m] * ws[c]) + b, act_out);
      }
    }
    __syncthreads();   // (the next row group overwrites xs)
  }
}

}  // namespace

extern "C" int sf_quantize_fp8(const void* x, int ldx, int M, int K, int rows_per_segment, void* q_out, float* scale_out, void* stream) {
  SF_CHECK(x && q_out && scale_out, "sf_quantize_fp8: null tensor");
  SF_CHECK(M > 0 && K > 0 && K % 8 == 0 && ldx >= K && ldx % 8 == 0, "sf_quantize_fp8: bad shape M=%d K=%d ldx=%d (K, ldx multiples of 8)", M, K, ldx);
  SF_CHECK(rows_per_segment > 0, "sf_quantize_fp8: rows_per_segment must be positive");
  SF_CHECK((uintptr_t)x % 16 == 0 && (uintptr_t)q_out % 8 == 0, "sf_quantize_fp8: misaligned tensor");
  const int segs = (M + rows_per_segment - 1) / rows_per_segment;
  SF_CHECK(segs <= 65535, "sf_quantize_fp8: %d segments exceed the grid limit", segs);
  // workgroups per segment: ~2 chunks of 8 per thread, at most PARTS (the scratch slots).  Measured: capped at 64
  // workgroups per segment the two passes over a [4680, 8960] input took 313 us (64 workgroups cannot keep HBM busy)
  const long chunks = (long)min(rows_per_segment, M) * (K / 8);
  const int parts = (int)std::min<long>(PARTS, std::max<long>(1, (chunks + 2 * QT - 1) / (2 * QT)));
  float* partial = scale_out + segs;
  const dim3 grid(parts, segs);
  SF_TRY(sf_launch<&fp8_amax_kernel>("sf_quantize_fp8", grid, dim3(QT), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, M, K, rows_per_segment, parts, partial));
  return sf_launch<&fp8_quantize_kernel>("sf_quantize_fp8", grid, dim3(QT), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, M, K, rows_per_segment, parts,
                                         (const float*)partial, (uint8_t*)q_out, scale_out);
}

extern "C" int sf_small_linear_fp8(const void* x, const void* w_q, const float* w_scale, const void* bias, void* out, int M, int N,
                                   int K, int rows_per_segment, int act_in, int act_out, void* stream) {
  SF_CHECK(x && w_q && w_scale && out, "sf_small_linear_fp8: null tensor");
  SF_CHECK(M > 0 && M <= 32 && N > 0 && K > 0 && K % 8 == 0, "sf_small_linear_fp8: unsupported shape M=%d N=%d K=%d (M<=32, K%%8==0)", M, N, K);
  SF_CHECK(rows_per_segment > 0, "sf_small_linear_fp8: rows_per_segment must be positive");
  SF_CHECK(act_in >= 0 && act_in <= 2 && act_out >= 0 && act_out <= 2, "sf_small_linear_fp8: bad activation code");
  SF_CHECK((uintptr_t)x % 2 == 0 && (uintptr_t)w_q % 8 == 0, "sf_small_linear_fp8: misaligned tensor");
  const size_t lds = 64 * sizeof(float) + (size_t)SLF_MB * K * 2;
  constexpr int LDS_CAP = 160 * 1024;   // the kernel's cap: the most any admitted K asks for
  SF_CHECK(lds <= LDS_CAP, "sf_small_linear_fp8: K=%d too large for the LDS activation stage", K);
  const int waves = (N + SLF_NPW - 1) / SLF_NPW;
  const dim3 grid((waves + SLF_THREADS / 64 - 1) / (SLF_THREADS / 64));
  return sf_launch<&small_linear_fp8_kernel, LDS_CAP>("sf_small_linear_fp8", grid, dim3(SLF_THREADS), lds, (hipStream_t)stream, (const bf16_t*)x,
                                                      (const uint8_t*)w_q, w_scale, (const bf16_t*)bias, (bf16_t*)out, M, N, K, rows_per_segment, act_in,
                                                      act_out);
}
