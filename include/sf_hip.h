/* sf_hip.h -- C-ABI of the MI355X (gfx950) implementation of Self-Forcing's chunk-wise
 * autoregressive denoising hot path.
 *
 * The reference (alazarteka/Self-Forcing) is pure Python/PyTorch and has no FFI layer of
 * its own: the path sits behind `WanDiffusionWrapper.forward` (utils/wan_wrapper.py:253-349)
 * and `CausalWanModel._forward_inference` (wan/modules/causal_model.py:725-893), whose heavy
 * ops go to third-party kernels (flash_attn, cuBLAS, cuDNN).  Each entry point below replaces
 * one of those op sequences; the citation on each says which.  `INTEGRATION.md` shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - every tensor is bf16 (uint16 storage) unless stated; row-major; strides in ELEMENTS;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream), allocates nothing, never synchronises, reads no environment variables and keeps no
 *     state between calls (apart from a per-device record that a kernel's LDS cap has been registered with
 *     the runtime, kept lock-free, so any thread may make a kernel's first call on any device);
 *   - return 0 on success, negative on error; `sf_last_error()` gives a thread-local message.
 */
#ifndef SF_HIP_H
#define SF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_HIP_ABI_VERSION 11

int sf_abi_version(void);
const char* sf_last_error(void);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue: out[M,N] = epi(a[M,K] @ w[N,K]^T + bias[N]).
 * Replaces nn.Linear (cuBLAS) + the elementwise ops that follow it in
 * wan/modules/causal_model.py:112-114 (q/k/v), :240 (o), :277-279 (ffn), :320/:331 (gated
 * residual), model.py:172-193 (cross-attention projections), causal_model.py:366 (head).
 * fp32 accumulation on the matrix cores; one rounding to bf16 at the store. */
enum sf_epilogue {
  SF_EPI_BIAS = 0,            /* y                                             */
  SF_EPI_BIAS_GELU = 1,       /* gelu_tanh(y)                                  */
  SF_EPI_BIAS_RESID = 2,      /* resid + y                                     */
  SF_EPI_BIAS_GATE_RESID = 3, /* resid + y * (gate_mod[n] + gate_e0[group(m)][n]) */
  SF_EPI_F32 = 4              /* raw fp32 accumulators, no bias: `out` is float*, ldo in floats
                                 (attention logits of the VAE's single-head block) */
};

typedef struct sf_gemm_args {
  const void* a;       /* [M, K], row stride lda                       */
  const void* w;       /* [N, K], row stride ldw (nn.Linear.weight)    */
  const void* bias;    /* [N] or NULL                                  */
  void* out;           /* [M, N], row stride ldo                       */
  const void* resid;   /* [M, N], row stride ldr; may alias out        */
  const void* gate_mod; /* [N]   (block.modulation[:, 2 or 5])         */
  const void* gate_e0;  /* [groups, *] first element of the gate chunk */
  int64_t gate_group_stride; /* elements between consecutive groups in gate_e0 */
  int32_t rows_per_group;    /* group(m) = m / rows_per_group                   */
  int32_t M, N, K;
  int32_t lda, ldw, ldo, ldr;
  int32_t epilogue;    /* enum sf_epilogue */
  int32_t batch;       /* > 1: `batch` independent products; entry b uses a + b*a_bstride, w + b*w_bstride,
                          out + b*o_bstride, resid + b*r_bstride (elements; bias / gates shared); 0 or 1: one product */
  int64_t a_bstride, w_bstride, o_bstride, r_bstride;
  int32_t structure;   /* enum sf_gemm_structure: 0 = picked from the shape; the others force a tiling (tests, A/B timing) */
} sf_gemm_args;

enum sf_gemm_structure { SF_GEMM_AUTO = 0, SF_GEMM_T128 = 1 /* 128 x 128 tile, 4 waves, 2 workgroups / CU */,
                         SF_GEMM_PP256 = 2 /* 256 x 256 tile, 8 waves, the two waves of a SIMD half a phase apart */,
                         SF_GEMM_PP128 = 3 /* 128 x 256 tile, same structure, two phases per k-tile, 3-deep rings */,
                         SF_GEMM_PP224 = 4, SF_GEMM_PP192 = 5 /* the 256 x 256 kernel with 7 / 6 row tiles per wave: 224- and
                                                                 192-row tiles for shapes whose 256-row tiles leave a round of
                                                                 workgroups mostly empty */ };

int sf_gemm_bf16(const sf_gemm_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * FP8 linear layers (opt-in).  Replaces the reference's optional torchao quantisation of the
 * generator, `quantize_(transformer, Float8DynamicActivationFloat8WeightConfig(granularity=PerTensor()))`
 * (demo.py:277-283), whose F.linear calls then run as scaled fp8 matmuls.  Format: OCP e4m3fn (torch.float8_e4m3fn).
 * The recipe (ours, pinned by the tests; torchao is not reproduced bit for bit), for weights once at load and for
 * activations on every call, over one SEGMENT of rows (activations: the rows of one generator pass, all its samples):
 *   s = max(amax(|x|) as fp32, 1e-12) / 448,   q = e4m3fn_rne(clamp(x.float() / s, -448, 448))   (true fp32 division)
 *
 * sf_quantize_fp8: x [M, K] bf16 (row stride ldx) -> q_out [M, K] e4m3 (contiguous), scale_out[seg] = s of rows
 * [seg * rows_per_segment, (seg + 1) * rows_per_segment).  scale_out is float32 [segments * (1 + SF_FP8_AMAX_PARTS)]:
 * the scales, then scratch for the partial maxima (written and read by the call; the result does not depend on
 * the order of the reduction).  Two launches. */
#define SF_FP8_AMAX_PARTS 1024
int sf_quantize_fp8(const void* x, int ldx, int M, int K, int rows_per_segment, void* q_out, float* scale_out, void* stream);

/* out = epi(acc * (a_scale[m / rows_per_segment] * w_scale[n]) + bias[n]), acc the fp32 sum of the e4m3 products of
 * args->a [M, K] and args->w [N, K] (both e4m3; lda / ldw in bytes); one rounding to bf16.  Every epilogue but
 * SF_EPI_F32, every structure of sf_gemm_bf16 (bit-identical to each other; SF_GEMM_AUTO picks by the same rule),
 * no batch.  K % 128 == 0.  w_scale: fp32 [N], 16-byte aligned (a stacked q|k|v weight carries 3 values). */
int sf_gemm_fp8(const sf_gemm_args* args, const float* a_scale, int rows_per_segment, const float* w_scale, void* stream);

/* sf_small_linear on e4m3 weights w_q [N, K] with column scales w_scale [N]: the activation act_in(x) (rounded to
 * bf16) is quantised inside the kernel with one scale per segment of rows_per_segment rows, then
 * out = act_out(acc * (sa[seg(m)] * w_scale[n]) + bias[n]).  Replaces the time-embedding MLPs' F.linear under the
 * reference's fp8 quantisation (causal_model.py:464-467, :829-832; demo.py:277-283).  One launch. */
int sf_small_linear_fp8(const void* x, const void* w_q, const float* w_scale, const void* bias, void* out, int M, int N, int K,
                        int rows_per_segment, int act_in, int act_out, void* stream);

/* Small-M linear layer (M <= 32), weight-bandwidth bound: out = act_out(act_in(x) @ w^T + b).
 * Replaces the time-embedding MLPs, causal_model.py:464-467, :829-832.
 * act codes: 0 none, 1 SiLU, 2 GELU-tanh. */
int sf_small_linear(const void* x, const void* w, const void* bias, void* out, int M, int N, int K,
                    int act_in, int act_out, void* stream);

/* Sinusoidal timestep embedding in float64, wan/modules/model.py:15-25.
 * t: [n] float32 (t_is_int64 = 0) or int64 (= 1); out [n, dim] bf16 = cat(cos, sin). */
int sf_sinusoid_embedding(const void* t, int t_is_int64, void* out, int n, int dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm (no affine, eps) + AdaLN modulate: out = LN(x) * (1 + scale) + shift with
 * scale = mod_scale[c] + e0_scale[group(row)][c], shift likewise; group(row) = row / rows_per_group.
 * Replaces norm1/norm2/head.norm + the broadcast mul/add of causal_model.py:315, :327-328, :366. */
int sf_layernorm_modulate(const void* x, void* out, int M, int C, float eps, const void* mod_shift,
                          const void* mod_scale, const void* e0_shift, const void* e0_scale,
                          int64_t e0_group_stride, int rows_per_group, void* stream);

/* LayerNorm with affine weight/bias (norm3, causal_model.py:268-270, :324). */
int sf_layernorm_affine(const void* x, const void* weight, const void* bias, void* out, int M, int C,
                        float eps, void* stream);

/* WanRMSNorm over the full channel dim (model.py:70-86): out = bf16(x * rsqrt(mean(x^2)+eps)) * w.
 * x has row stride ldx, out row stride ldo (in place allowed). */
int sf_rmsnorm(const void* x, int ldx, const void* weight, void* out, int ldo, int M, int C, float eps,
               void* stream);

/* Fused q/k RMSNorm + 3-axis RoPE + KV-cache write for the fused qkv projection output
 * (causal_model.py:112-114, :195-200, :221-229).
 *   qkv   [B*L, 3C]  (q | k | v per row), L = f*h*w tokens per sample in (f,h,w) order
 *   q_out [B*L, C]   roped, normalised queries
 *   k_cache/v_cache [B, cache_tokens, H, D]: rows [write_start, write_start+L) are overwritten
 *   rope_cos/sin: float32 [1024, D/2] tables in the reference's `freqs` column layout
 *   (time | height | width), time index offset by start_frame. */
int sf_qkv_norm_rope_cache(const void* qkv, const void* norm_q_w, const void* norm_k_w, void* q_out,
                           void* k_cache, void* v_cache, const float* rope_cos, const float* rope_sin,
                           int B, int f, int h, int w, int C, int num_heads, int64_t cache_tokens,
                           int write_start, int start_frame, float eps, void* stream);

/* Rolling-window eviction, causal_model.py:212-217: for every sample move
 * cache[sink+evict : sink+evict+keep] -> cache[sink : sink+keep] (overlap-safe). */
int sf_kv_evict(void* cache, int B, int64_t cache_tokens, int row_elems, int sink, int evict, int keep,
                void* scratch, size_t scratch_bytes, void* stream);

/* Re-base the temporal RoPE of cached keys, in place: rows [row0, row0 + rows) of every sample of the bf16
 * [B, cache_tokens, num_heads, 128] cache are rotated back by delta_frames frames, so that a session can subtract
 * delta_frames from every temporal position it still holds (scores depend on pos_q - pos_k only).  Of each head only
 * the temporal pairs change -- complex pairs j < 22, columns 2j and 2j + 1, angles from table columns 0..21, the split
 * of sf_qkv_norm_rope_cache: with c = rope_cos[delta_frames][j], s = rope_sin[delta_frames][j] and (a, b) the pair,
 *   a' = bf16(fl(fl(a c) + fl(b s))),  b' = bf16(fl(fl(b c) - fl(a s)))
 * every fp32 operation rounded on its own, bf16 by round-to-nearest-even (rope_shift_reference.py; bit exact).
 * Columns 44..127, rows outside the range and V are never written.  1 <= delta_frames <= 1023; rows == 0 is a no-op.
 * No scratch. */
int sf_kv_rope_shift(void* k_cache, int B, int64_t cache_tokens, int num_heads, int64_t row0, int64_t rows,
                     const float* rope_cos, const float* rope_sin, int delta_frames, void* stream);

/* ------------------------------------------------------------------------------------------
 * Non-causal attention softmax(q k^T / sqrt(D)) v, D = 128.  Replaces flash_attn_varlen_func /
 * SDPA of wan/modules/attention.py:136-150, :198 for self-attention over the KV cache
 * (causal_model.py:230-234) and for T5 cross-attention (model.py:189).
 *   q   [B, Lq, H, D]  with token stride q_stride (elements) and batch stride q_bstride
 *   k,v [B, Lk, H, D]  with token stride kv_stride and batch stride kv_bstride
 *   out [B, Lq, H, D]  token stride o_stride, batch stride o_bstride
 * structure: SF_ATTN_AUTO picks from the shape (on Lk, not on the folded key counts); the others name the kernel
 *   (tests and A/B timing; every structure computes every shape): SF_ATTN_R64 = 64 query rows per wave, one wave per
 *   SIMD, hand-scheduled (256 rows per workgroup); SF_ATTN_W8 = 8-wave anti-phase workgroups of 256 rows; SF_ATTN_W4 =
 *   4-wave workgroups of 128 rows.
 * accumulate: out = bf16(float(out) + attention), the sum taken in fp32 in the kernel's epilogue and rounded once.  The
 *   i2v cross-attention (model.py:240-266) is o(attn(q, k, v) + attn(q, k_img, v_img)): the image attention accumulates
 *   into the buffer the text attention wrote, with no third buffer and no elementwise pass.  An epilogue variant of the
 *   SF_ATTN_W8 and SF_ATTN_W4 structures: SF_ATTN_AUTO picks between those two, SF_ATTN_R64 is an error.  Every query
 *   row of `out` must hold a finite value on entry.
 * keys / log2w (DEVICE arrays, int32 [B] / float [B], as sf_cross_fold_scan writes them; read by the kernels only): a key
 *   slab whose trailing rows repeat (a prompt's padding keys).  Sample b attends only rows [0, keys[b]) and log2w[b] is
 *   added to the exp2-domain score of row keys[b] - 1, which so stands for 2^log2w[b] identical rows.  Both NULL: every
 *   row.  Not built together with accumulate (an error). */
enum sf_attn_structure { SF_ATTN_AUTO = 0, SF_ATTN_R64 = 1, SF_ATTN_W8 = 2, SF_ATTN_W4 = 3 };

typedef struct sf_attention_args {
  const void *q, *k, *v;
  void* out;
  int32_t B, H, Lq, Lk;
  int64_t q_stride, q_bstride, kv_stride, kv_bstride, o_stride, o_bstride;
  int32_t structure;          /* enum sf_attn_structure */
  int32_t accumulate;         /* 1: out += attention */
  const int32_t* keys;        /* both or neither */
  const float* log2w;
} sf_attention_args;

int sf_attention(const sf_attention_args* args, void* stream);

/* Per layer l and sample b of the cross-attention caches ck / cv (HOST arrays [layers] of device pointers, each
 * [B, text_len, row_elems] bf16): same = the number of trailing rows that equal the last row bit for bit in BOTH caches;
 * keys[l * B + b] = text_len - same + 1 (the rows in front plus one representative; text_len when same == 1) and
 * log2w[l * B + b] = log2(same).  Zero-padded prompt embeddings give same = text_len - prompt length; any other cache
 * contents just fold less.  Nothing is read back to the host. */
int sf_cross_fold_scan(const void* const* ck_cache_host, const void* const* cv_cache_host, int layers, int B, int text_len,
                       int row_elems, int32_t* keys, float* log2w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch gather for the (1,2,2) Conv3d patch embedding, causal_model.py:458-459, :775-781:
 * x [B, F, Cin, H, W] (the wrapper's layout) -> cols [B*F*(H/2)*(W/2), Cin*4] with column index
 * c*4 + p*2 + q, so that cols @ patch_embedding.weight.flatten(1)^T is the convolution. */
int sf_patchify(const void* x, void* cols, int B, int F, int Cin, int H, int W, void* stream);

/* Unpatchify (causal_model.py:1081-1104) fused with flow -> x0 (wan_wrapper.py:204-228):
 *   head_out [B*F*h*w, 4*Cout] (column = (p*2+q)*Cout + c) -> flow [B, F, Cout, H, W],
 *   x0 = xt - sigma(t) * flow evaluated in float64; sigma by nearest-timestep lookup in the
 *   n_table-entry float32 tables.  timestep has B*groups entries (frames_per_group = F/groups). */
int sf_unpatchify_x0(const void* head_out, const void* xt, const void* timestep, int t_is_int64,
                     const float* sigmas, const float* timesteps, int n_table, void* flow, void* x0,
                     int B, int F, int groups, int Cout, int H, int W, void* stream);

/* FlowMatchScheduler.add_noise (utils/scheduler.py:159-176): out = (1-sigma) x0 + sigma eps in
 * fp32; one timestep per leading index (n_outer), inner = C*H*W elements each. */
int sf_add_noise(const void* x0, const void* eps, const void* timestep, int t_is_int64,
                 const float* sigmas, const float* timesteps, int n_table, void* out, int n_outer,
                 int64_t inner, void* stream);

/* out[i] = sum_{k < n_terms} coefs[k] * xs[k][i]   (bf16 tensors of n elements, fp32 accumulation in the order
 * k = 0, 1, ...; one rounding to bf16 at the end; 1 <= n_terms <= SF_LINCOMB_MAX; `out` may alias any input).
 * `xs` and `coefs` are HOST arrays (device pointers / scalars), read before the call returns.
 * Replaces the tensor arithmetic of the 50-step sampler: the classifier-free-guidance blend
 * (pipeline/causal_diffusion_inference.py:423-424) and FlowUniPCMultistepScheduler's convert_model_output /
 * multistep_uni_p_bh_update / multistep_uni_c_bh_update (wan/utils/fm_solvers_unipc.py:279-347, :350-484, :486-626),
 * all of which are linear in their tensors with scalar coefficients the host evaluates. */
#define SF_LINCOMB_MAX 6
int sf_lincomb_bf16(void* out, const void* const* xs, const float* coefs, int n_terms, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * One whole denoiser pass: CausalWanModel._forward_inference + flow->x0
 * (causal_model.py:725-893, wan_wrapper.py:288-300, :340-344) as a single host call that
 * enqueues every kernel on `stream`. */
typedef struct sf_layer_weights {
  const void* modulation;                 /* [6, C] */
  const void *norm3_w, *norm3_b;          /* [C]    */
  const void *qkv_w, *qkv_b;              /* [3C, C], [3C]: self_attn q|k|v stacked */
  const void *norm_q_w, *norm_k_w;        /* [C]    */
  const void *o_w, *o_b;                  /* [C, C] */
  const void *cq_w, *cq_b;                /* cross_attn.q */
  const void *ckv_w, *ckv_b;              /* [2C, C]: cross_attn k|v stacked */
  const void *cnorm_q_w, *cnorm_k_w;
  const void *co_w, *co_b;
  const void *ffn0_w, *ffn0_b;            /* [ffn, C] */
  const void *ffn2_w, *ffn2_b;            /* [C, ffn] */
} sf_layer_weights;

typedef struct sf_model {
  int32_t dim, ffn_dim, num_heads, num_layers, in_dim, out_dim, freq_dim, text_dim, text_len;
  float eps;
  const void *patch_w, *patch_b;          /* [C, in_dim*4] */
  const void *text0_w, *text0_b, *text2_w, *text2_b;
  const void *time0_w, *time0_b, *time2_w, *time2_b;
  const void *tproj_w, *tproj_b;          /* [6C, C] */
  const void *head_w, *head_b;            /* [4*out_dim, C] */
  const void* head_mod;                   /* [2, C] */
  const void *pose_w, *pose_b;            /* optional pose_proj Linear(pose_dim, C) (causal_model.py:493-503); NULL if absent */
  int32_t pose_dim;                       /* width of add_condition; with pose_w == NULL and pose_dim == dim the projection is
                                             the reference's nn.Identity() of dim-5120 models (:500-501): x += add_condition */
  const sf_layer_weights* layers_host;    /* HOST array [num_layers] */
  const float *rope_cos, *rope_sin;       /* float32 [1024, 64] */
  const float *sched_sigmas, *sched_timesteps; /* float32 [n_table] */
  int32_t n_table;
  /* ---- ABI 10: FP8 linear layers (sf_gemm_fp8).  All zero = bf16 (the fields above).  With fp8 = 1 every nn.Linear of
   * the reference's CausalWanModel reads the e4m3 weight *_q [N, K] and its fp32 column scales *_s [N] instead of the
   * bf16 *_w (which may then be NULL); the patch embedding (a Conv3d) stays bf16.  Activations are quantised per pass. */
  int32_t fp8;
  const void *text0_q, *text2_q, *time0_q, *time2_q, *tproj_q, *head_q, *pose_q;
  const float *text0_s, *text2_s, *time0_s, *time2_s, *tproj_s, *head_s, *pose_s;
  const struct sf_layer_fp8* layers_fp8_host;   /* HOST array [num_layers] */
} sf_model;

typedef struct sf_layer_fp8 {             /* e4m3 weights [N, K] + fp32 column scales [N] of one block */
  const void *qkv_q, *o_q, *cq_q, *ckv_q, *co_q, *ffn0_q, *ffn2_q;
  const float *qkv_s, *o_s, *cq_s, *ckv_s, *co_s, *ffn0_s, *ffn2_s;
} sf_layer_fp8;

typedef struct sf_forward_args {
  int32_t batch, frames, lat_h, lat_w;    /* noisy: [B, F, in_dim, H, W] */
  int32_t groups;                         /* timestep.shape[1] (modulation groups)       */
  const void* noisy;
  const void* timestep;                   /* [B, groups] */
  int32_t t_is_int64;
  const void* prompt_embeds;              /* [B, text_len, text_dim], zero padded; read only if init_cross */
  int32_t init_cross;                     /* 1: (re)compute text embedding + cross-attn K/V caches */
  const void* add_condition;              /* optional pose tokens [B, F*h*w, pose_dim]: x += pose_proj(add_condition)
                                             after the patch embedding (causal_model.py:786-819); NULL if none */
  void* const* k_cache_host;              /* HOST arrays [num_layers] of device pointers */
  void* const* v_cache_host;              /*   each [B, cache_tokens, H, D]              */
  void* const* ck_cache_host;             /*   each [B, text_len, H, D]                  */
  void* const* cv_cache_host;
  int64_t cache_tokens;
  /* cache plan (host integers; see kv_cache_plan in self-forcing_amd/kvcache.py) */
  int32_t sink_tokens, evict, keep;       /* evict > 0: roll the window first */
  int32_t write_start;                    /* rows [write_start, write_start + F*h*w) get the new K/V */
  int32_t attn_start, attn_end;           /* attend over cache rows [attn_start, attn_end) */
  int32_t start_frame;                    /* RoPE time offset = current_start // (h*w) */
  void* evict_scratch;                    /* >= batch * keep * dim * 2 bytes when evict > 0 */
  size_t evict_scratch_bytes;
  int32_t cache_only;                     /* 1: only the KV-cache update is wanted (the context pass /
                                             warm-up passes, whose outputs the pipeline discards,
                                             causal_inference.py:143-168, :227-235): everything after
                                             the LAST layer's K/V write is skipped, outputs untouched */
  void* flow_out;                         /* [B, F, out_dim, H, W] */
  void* x0_out;                           /* [B, F, out_dim, H, W] */
  void* workspace;
  size_t workspace_bytes;
  void* kv_index_out;                     /* optional int64 [num_layers][2]: every row is set to (global_end, attn_end) at
                                             the end of the pass -- the cache dicts' "global_end_index" / "local_end_index"
                                             tensors (causal_model.py:235-236) when they are views of one buffer; NULL:
                                             the caller updates its index tensors itself */
  int64_t global_end;                     /* current_start + F*h*w (only written to kv_index_out) */
} sf_forward_args;

/* ------------------------------------------------------------------------------------------
 * The i2v model type (CausalWanModel(model_type='i2v', in_dim=36), causal_model.py:767-775, :844-846; WanI2VCrossAttention
 * and MLPProj, model.py:222-266, :469-481).  Everything i2v travels in the structs below, beside an sf_model /
 * sf_forward_args pair that keeps its layout:
 *   patch embedding  cat([x, y], channel) = 16 + 20 = 36 channels -> 144 columns, zero-padded to the GEMM's K % 64 == 0:
 *                    the sf_model of an i2v generator says in_dim = 48 and carries patch_w [dim, 192] with columns
 *                    144..191 zero; `noisy` stays [B, F, 16, H, W]
 *   context          img_emb(clip_feature) -> 257 image tokens, once per prompt (init_cross)
 *   cross-attention  out = o(attn(q, k, v) + attn(q, k_img, v_img)), k_img = norm_k_img(k_img(ctx_img)), v_img = v_img(ctx_img),
 *                    both cached per layer beside the text K / V. */

/* The 36-channel patch gather: x [B, F, x_channels, H, W] -> columns c * 4 + p * 2 + q (c < x_channels) of cols
 * [B*F*(H/2)*(W/2), pad_channels * 4]; y [B, y_channels, F, H, W] CHANNEL-first through its element strides (batch, channel,
 * frame; H x W planes contiguous; y_bstride 0 = one image for the whole batch) -> channels x_channels ..; the remaining
 * channels up to pad_channels are written as zeros. */
int sf_patchify_i2v(const void* x, const void* y, void* cols, int B, int F, int x_channels, int y_channels, int pad_channels,
                    int H, int W, int64_t y_bstride, int64_t y_cstride, int64_t y_fstride, void* stream);

/* nn.LayerNorm with affine weight / bias over rows of any width C % 8 == 0 (bf16 in / out, fp32 statistics):
 * img_emb.proj.0 normalises clip_dim = 1280, which sf_layernorm_affine (C = 512 * {1,2,3,4,5,6,8,10}) cannot hold. */
int sf_layernorm_rows(const void* x, const void* weight, const void* bias, void* out, int M, int C, float eps, void* stream);

/* A chunk of the conditioning tensor y of an i2v generator, in one launch: y[c][t] (bf16, H x W planes contiguous, channel c
 * at y + c * y_cstride, frame t at + t * y_fstride elements: a frame range of a longer [C, F, h, w] buffer) =
 *   c <  mask_channels   1 when first_is_frame0 and t == 0, else 0                  (the "frame is known" mask)
 *   c >= mask_channels   bf16(latent[t][c - mask_channels])                          latent: fp32 [frames, latent_channels, h, w],
 *                                                                                    the rows sf_vae_encode_frames writes
 * and, with ref_map (bf16 [h, w, mask_channels + latent_channels] channels-last, as sf_pose_embed_ref writes it; NULL: none),
 * bf16(float(that value) + float(ref_map[.][c])): two roundings, what `cat([mask, latent]).to(bf16) + map` computes. */
int sf_i2v_assemble_y(const void* latent, const void* ref_map, void* y, int frames, int mask_channels, int latent_channels, int h, int w,
                      int64_t y_cstride, int64_t y_fstride, int first_is_frame0, void* stream);

typedef struct sf_i2v_layer {             /* WanI2VCrossAttention beyond WanT2VCrossAttention */
  const void *kvimg_w, *kvimg_b;          /* [2C, C], [2C]: cross_attn k_img|v_img stacked */
  const void* norm_k_img_w;               /* [C] */
} sf_i2v_layer;

typedef struct sf_i2v_model {
  int32_t clip_dim, clip_len;             /* clip_feature: [B, clip_len, clip_dim]; clip_dim % 64 == 0 */
  float img_eps;                          /* eps of img_emb's two LayerNorms (nn.LayerNorm's default 1e-5) */
  const void *img_ln0_w, *img_ln0_b;      /* img_emb.proj.0  LayerNorm(clip_dim)        */
  const void *img_fc1_w, *img_fc1_b;      /* img_emb.proj.1  Linear(clip_dim, clip_dim), then erf-GELU */
  const void *img_fc2_w, *img_fc2_b;      /* img_emb.proj.3  Linear(clip_dim, dim)      */
  const void *img_ln1_w, *img_ln1_b;      /* img_emb.proj.4  LayerNorm(dim)             */
  const sf_i2v_layer* layers_host;        /* HOST array [num_layers] */
} sf_i2v_model;

typedef struct sf_i2v_args {
  const void* clip_feature;               /* bf16 [B, clip_len, clip_dim]; read only with init_cross */
  const void* y;                          /* bf16 [B or 1, y_channels, F, H, W] of THIS pass's frames, through its strides */
  int64_t y_bstride, y_cstride, y_fstride;/* elements; y_bstride 0 broadcasts one image over the batch */
  int32_t y_channels;                     /* 16 + y_channels must be the generator's in_dim (36) */
  void* const* kimg_cache_host;           /* HOST arrays [num_layers] of device pointers, each [B, clip_len, H, D] bf16: */
  void* const* vimg_cache_host;           /*   written with init_cross, read by every pass                              */
} sf_i2v_args;

/* One call of the denoiser: one pass, or two passes of the rollout.
 * Two passes are the context pass of chunk k (passes[0], cache_only = 1: it rewrites the chunk's K / V "clean",
 * causal_inference.py:226-235) and the first denoising pass of chunk k + 1 (passes[1], :190-205), which the reference
 * runs back to back.  Layer l of the second needs only layer l's K / V of the first, so the two run layer by layer as one
 * batch of 2 x batch samples through every row-wise kernel and GEMM (twice the rows per GEMM) and one after the other
 * through the cache (eviction, K / V write, attention): bit-identical to two one-pass calls.  Both passes must name the
 * same caches, latent geometry, batch and groups, and the same workspace, sized for 2 x batch; neither may have
 * init_cross set; passes[1]->kv_index_out (if any) receives the final indices.
 * cross_keys (int32) / cross_log2w (float): device arrays [num_layers][batch] that belong to the cross-attention caches,
 * folding the prompt's padding keys.  A pass with init_cross fills them (sf_cross_fold_scan) behind the caches; every
 * pass hands layer l's slices to its cross-attention.  Caches filled by anything else need one sf_cross_fold_scan first.
 * Both NULL: every text key is attended.
 * i2v_model / i2v_args: an i2v generator's weights and this pass's image tensors: the 36-channel patch embedding and,
 * behind every layer's text cross-attention, the accumulating attention over the clip_len image keys.  With init_cross
 * the image context and every layer's k_img / v_img are computed beside the text K / V.  Not built: two passes and fp8
 * Linears (model->fp8 != 0) of an i2v generator; both are errors. */
typedef struct sf_forward_call {
  const sf_forward_args* passes[2];       /* cache_only passes first */
  int32_t n_passes;                       /* 1 or 2 */
  int32_t* cross_keys;                    /* both or neither; written only by a pass with init_cross */
  float* cross_log2w;
  const sf_i2v_model* i2v_model;          /* both or neither; NULL: a t2v generator */
  const sf_i2v_args* i2v_args;
} sf_forward_call;

int sf_dit_forward(const sf_model* model, const sf_forward_call* call, void* stream);
/* Bytes of sf_forward_args.workspace for one pass of `batch` samples (two passes: 2 x batch); with i2v_model (NULL: a
 * t2v generator) the image context's buffers behind them.  0 for a bad shape. */
size_t sf_dit_workspace_bytes(const sf_model* model, const sf_i2v_model* i2v_model, int batch, int frames, int lat_h, int lat_w,
                              int groups);

/* ==========================================================================================
 * Wan VAE decode (latents -> pixels): WanVAEWrapper.decode_to_pixel -> WanVAE_.decode /
 * cached_decode -> Decoder3d.forward (utils/wan_wrapper.py:95-117, wan/modules/vae.py:556-593,
 * :423-472).  Activations are CHANNELS-LAST bf16 volumes [T][H][W][C]; the reference's
 * `feat_cache` list (two cached input frames per causal convolution, vae.py:206-216) becomes two
 * history frames kept physically in front of the new frames of each convolution's input buffer.
 * ========================================================================================== */

/* Implicit-GEMM convolution, fp32 accumulation on the matrix cores:
 *   out[(t,h,w)][n] = bias[n] + sum_{dt,dh,dw,ci} x[t+dt+t_in_offset][(h+dh-kh/2)>>up][(w+dw-kw/2)>>up][ci]
 *                                               * w[n][((dt*kh+dh)*kw+dw)*Cin + ci]
 * with zero padding in h/w.  Replaces CausalConv3d (vae.py:17-38; kernel 3x3x3, (3,1,1) or 1x1x1),
 * Resample's nearest-2x Upsample + Conv2d 3x3 (vae.py:77-83, :139-141; upsample = 1, kt = 1),
 * the residual add of ResidualBlock (vae.py:221), the channel->frame interleave after the time
 * convolution (vae.py:134-137) and the .float().clamp_(-1, 1) of decode_to_pixel (wan_wrapper.py:113). */
enum sf_conv_epilogue {
  SF_CONV_BIAS = 0,            /* bf16 out[row][n] = y                                            */
  SF_CONV_BIAS_RESID = 1,      /* bf16 out[row][n] = y + resid[row][n]; resid may alias out       */
  SF_CONV_BIAS_CLAMP_F32 = 2   /* float out_f32[t][n][h][w] = clamp(y, -1, 1) (planar, Cout small) */
};

typedef struct sf_conv_args {
  const void* x;          /* [Tin][Hin][Win][Cin], Cin % 32 == 0                                   */
  const void* w;          /* [Cout][ldw]: k = tap*Cin + ci, zero padded to ldw >= roundup(taps*Cin, 64) */
  const void* bias;       /* [Cout]                                                                */
  void* out;              /* rows of ldo channels; row = (out_frame_offset + t')*H*W + h*W + w     */
  const void* resid;      /* same row indexing, ldr channels per row                               */
  float* out_f32;         /* SF_CONV_BIAS_CLAMP_F32 only: [Tout][Cout][H][W]                       */
  int32_t Tout, H, W;     /* output volume                                                         */
  int32_t Hin, Win;       /* input frame size: (H, W), or (H/2, W/2) when upsample = 1             */
  int32_t Cin, Cout;
  int32_t kt, kh, kw;     /* 3 or 1 each; kh == kw                                                 */
  int32_t upsample;       /* 1: read the input through a nearest-neighbour 2x upsampling           */
  int32_t t_in_offset;    /* input frame of tap dt for output frame t is t + dt + t_in_offset      */
  int32_t ldw, ldo, ldr;
  int32_t out_frame_offset;
  int32_t interleave_c;   /* > 0 (= Cout/2): channel n of output frame t goes to frame 2t + n/interleave_c,
                             channel n % interleave_c (t' above)                                   */
  int32_t epilogue;       /* enum sf_conv_epilogue */
  int32_t structure;      /* enum sf_conv_structure: 0 = picked from the shape; the others force a kernel (tests, A/B timing) */
  /* Optional second output of the SF_CONV_HALO kernel with Cout = 96 or 192 (all channels in one tile): the NEXT
   * convolution's input, SiLU(RMS_norm(y) * gamma) (vae.py:41-56, :190-196), written to
   * norm_out[((norm_frame_offset + t) * H + h) * W + w][norm_ld]; `out` may then be NULL (raw result not needed). */
  void* norm_out;
  const void* norm_gamma; /* [Cout] */
  int32_t norm_ld, norm_frame_offset;
  /* Strided input gathers of the encoder's downsampling (Resample 'downsample2d/3d', vae.py:87-97, :143-160); 0 = 1 = none.
   * stride_hw = 2: ZeroPad2d((0,1,0,1)) + 3x3 stride 2 (kh = kw = 3, no upsample): output (h, w) reads input
   *                (2h + dh, 2w + dw), zero past the right / bottom edge; H = Hin / 2, W = Win / 2 (floor).
   * stride_t = 2:  output frame t reads input frames 2t + dt + t_in_offset (the (3,1,1) time convolution, no padding).
   * The halo structure takes neither (AUTO falls back to the implicit GEMM). */
  int32_t stride_hw, stride_t;
} sf_conv_args;

enum sf_conv_structure { SF_CONV_AUTO = 0, SF_CONV_IGEMM = 1 /* A tile gathered per tap (every shape) */,
                         SF_CONV_HALO = 2 /* 16 x 16 output patch, input halo staged once per (channel slice, frame):
                                             3 x 3 spatial taps, Cout % 96 == 0, bf16 bias / bias + residual */ };

int sf_conv_igemm(const sf_conv_args* args, void* stream);
int sf_conv_pick_nt(int cout);   /* column tiles (of 16) per wave the launcher will use for Cout    */

/* RMS_norm of the VAE (vae.py:41-56): out = x / max(||x||_2, 1e-12) * sqrt(C) * gamma over the C
 * channels of each row, optionally followed by SiLU (the nn.SiLU after it in ResidualBlock / head,
 * vae.py:190-196, :420-421).  x, out: [rows][C] contiguous, C % 8 == 0, C <= 512; in place allowed. */
int sf_rmsnorm_silu_cl(const void* x, const void* gamma, void* out, int64_t rows, int C, int silu,
                       void* stream);

/* Row softmax of the single-head attention block (vae.py:252-257): p[r][c] = softmax_c(scale * s[r][c])
 * for c < cols, 0 for cols <= c < cols_padded.  s float32 row stride lds, p bf16 row stride ldp. */
int sf_softmax_rows(const float* s, int64_t lds, void* p, int64_t ldp, int rows, int cols,
                    int cols_padded, float scale, void* stream);

/* Latent frame -> input of decoder.conv1: un-scale (z * std + mean, vae.py:559-563), the 1x1x1
 * conv2 (vae.py:564) and the layout change [z][h][w] -> [h][w][c_pad] (channels z..c_pad-1 zero). */
int sf_vae_prepare_latent(const void* latent, const float* mean, const float* std, const void* conv2_w,
                          const void* conv2_b, void* out, int z, int h, int w, int c_pad, void* stream);

typedef struct sf_vae_conv {
  const void* w;          /* repacked [cout][ldw] as sf_conv_args.w; NULL = layer absent           */
  const void* bias;       /* [cout] */
  int32_t cin, cout, kt, kh, kw, ldw;   /* cin already padded to a multiple of 32                  */
} sf_vae_conv;

typedef struct sf_vae_resblock {          /* ResidualBlock, vae.py:182-221 */
  const void* gamma1;     /* residual.0.gamma [in_dim]  */
  const void* gamma2;     /* residual.3.gamma [out_dim] */
  sf_vae_conv conv1;      /* residual.2 */
  sf_vae_conv conv2;      /* residual.6 */
  sf_vae_conv shortcut;   /* 1x1x1, w = NULL when in_dim == out_dim */
} sf_vae_resblock;

#define SF_VAE_MAX_STAGES 4

typedef struct sf_vae_model {             /* Decoder3d + conv2, vae.py:369-421, :503 */
  int32_t z_dim;
  int32_t n_stages;                       /* len(dim_mult) = 4                                      */
  int32_t res_per_stage;                  /* num_res_blocks + 1 = 3                                 */
  int32_t temporal_up[SF_VAE_MAX_STAGES]; /* stage i ends with upsample3d (1) / upsample2d (0); last stage: none */
  const float* latent_mean;               /* float32 [z_dim] */
  const float* latent_std;                /* float32 [z_dim] */
  const void *conv2_w, *conv2_b;          /* [z][z], [z] */
  sf_vae_conv conv1;                      /* decoder.conv1, cin padded to 32 */
  sf_vae_resblock mid0, mid2;             /* decoder.middle.0 / .2 */
  const void* attn_gamma;                 /* middle.1.norm.gamma [C]            */
  const void *attn_qk_w, *attn_qk_b;      /* to_qkv rows [0, 2C): [2C][C], [2C] */
  const void *attn_v_w, *attn_v_b;        /* to_qkv rows [2C, 3C)               */
  const void *attn_proj_w, *attn_proj_b;  /* [C][C], [C] */
  const sf_vae_resblock* res_host;        /* HOST array [n_stages * res_per_stage] */
  sf_vae_conv time_conv[SF_VAE_MAX_STAGES];   /* per stage; w = NULL where absent  */
  sf_vae_conv up_conv[SF_VAE_MAX_STAGES];     /* Resample.resample[1] (Conv2d 3x3) */
  const void* head_gamma;                 /* decoder.head.0.gamma */
  sf_vae_conv head_conv;                  /* decoder.head.2 (cout = 3) */
} sf_vae_model;

/* Per-stream persistent state = the input volumes of every cached convolution: 2 history frames + new frames, as a
 * window that slides through 2 + window_frames * T frames (T = the stage's frames per latent frame); scratch =
 * everything else, reusable by any stream that does not overlap in time.  `window_frames` (2..64) is chosen by the
 * caller once per state: a call decodes up to window_frames - 1 latent frames. */
size_t sf_vae_state_bytes(const sf_vae_model* model, int lat_h, int lat_w, int window_frames);
size_t sf_vae_scratch_bytes(const sf_vae_model* model, int lat_h, int lat_w, int window_frames);
/* WanVAE_.clear_cache (vae.py:610-617): zero every history. */
int sf_vae_reset(const sf_vae_model* model, void* state, size_t state_bytes, int lat_h, int lat_w,
                 int window_frames, void* stream);
/* n_frames iterations of the per-latent-frame loop of decode / cached_decode (vae.py:566-578) in one call:
 * latent_frames [n_frames][z][lat_h][lat_w] bf16 -> pixels [T][3][8 lat_h][8 lat_w] float32 in [-1, 1], T = 1 for
 * the frame that follows a reset (frame_index 0: decoded alone, vae.py:109-111, :134-137), else 4 n_frames.  The
 * result is bit-identical to n_frames single-frame calls (the causal convolutions see the same inputs either way); a
 * group fills the chip at the low-resolution stages.
 * The library keeps no state of its own, so the caller says where the history windows are: `frame_index` = latent
 * frames decoded into `state` since its reset; `window` = the slot (in latent frames) this call's frames take in the
 * current lap of the sliding windows, window + n_frames <= window_frames; `history_at` = where the previous call
 * ended: equal to `window` while the windows slide on, or -- when the caller restarts at window 0 because the frames
 * no longer fit -- the previous lap's end slot, from which the two history frames of every volume are first copied
 * to the front.  A caller's bookkeeping (self-forcing_amd/vae.py): slot = 0 after a reset; per call: if slot +
 * n_frames > window_frames: (window, history_at) = (0, slot) else (slot, slot); slot = window + n_frames. */
int sf_vae_decode_frames(const sf_vae_model* model, void* state, size_t state_bytes, void* scratch,
                         size_t scratch_bytes, const void* latent_frames, int lat_h, int lat_w, int window_frames,
                         int frame_index, int n_frames, int window, int history_at, float* pixels_out, void* stream);

/* ==========================================================================================
 * Wan VAE encode (pixels -> latents): WanVAEWrapper.encode_to_latent -> WanVAE_.encode -> Encoder3d.forward with
 * feat_cache (utils/wan_wrapper.py:78-92, wan/modules/vae.py:517-543, :265-367).  Same volumes and history model as
 * the decoder: every causal convolution keeps two history frames physically in front of its new frames; the (3,1,1)
 * stride-2 time convolution of 'downsample3d' reads the last of them (its one-frame cache, vae.py:143-160).
 * ========================================================================================== */

/* One sample's pixel frames, channels-first [3][T][H][W] (bf16, or float32 when is_f32; pixel (c, t, y, x) at
 * pixels[c * c_stride + (t * H + y) * W + x]) -> channels-last bf16 [T][H][W][c_pad], channels 3..c_pad-1 zero
 * (the input of encoder.conv1, vae.py:324-336). */
int sf_vae_prepare_pixels(const void* pixels, int is_f32, int64_t c_stride, void* out, int T, int H, int W, int c_pad,
                          void* stream);

/* Head output [T][h][w][ld_in] bf16 -> the 1x1x1 conv1 rows 0..z-1 (mu, vae.py:538; fp32 accumulation), then
 * (mu - mean[c]) * (1 / std[c]) (vae.py:539-542) -> float32 [T][z][h][w].  conv1_w [z][ld_w] bf16 (the first z rows
 * of the 2z x 2z weight, ld_w >= cin), conv1_b [z]. */
int sf_vae_finish_latent(const void* head_out, int ld_in, int cin, const void* conv1_w, int ld_w, const void* conv1_b,
                         const float* mean, const float* std, float* out, int T, int z, int h, int w, void* stream);

typedef struct sf_vae_encoder {           /* Encoder3d + conv1, vae.py:265-367, :502 */
  int32_t z_dim;                          /* latent channels (mu) = 16; the head writes 2 z_dim                       */
  int32_t n_stages;                       /* len(dim_mult) = 4                                                         */
  int32_t res_per_stage;                  /* num_res_blocks = 2                                                        */
  int32_t temporal_down[SF_VAE_MAX_STAGES]; /* stage i ends with downsample3d (1) / downsample2d (0); last stage: none */
  const float* latent_mean;               /* float32 [z_dim] */
  const float* latent_std;                /* float32 [z_dim] */
  const void *conv1_w, *conv1_b;          /* WanVAE_.conv1 rows [0, z_dim): [z_dim][2 z_dim], [z_dim]   */
  sf_vae_conv in_conv;                    /* encoder.conv1 (3 -> dims[0]), cin padded to 32              */
  const sf_vae_resblock* res_host;        /* HOST array [n_stages * res_per_stage]: encoder.downsamples  */
  sf_vae_conv down_conv[SF_VAE_MAX_STAGES];   /* Resample.resample[1] (Conv2d 3x3 stride 2)              */
  sf_vae_conv time_conv[SF_VAE_MAX_STAGES];   /* (3,1,1) stride 2; w = NULL where absent                 */
  sf_vae_resblock mid0, mid2;             /* encoder.middle.0 / .2 */
  const void* attn_gamma;                 /* middle.1.norm.gamma [C]            */
  const void *attn_qk_w, *attn_qk_b;      /* to_qkv rows [0, 2C): [2C][C], [2C] */
  const void *attn_v_w, *attn_v_b;        /* to_qkv rows [2C, 3C)               */
  const void *attn_proj_w, *attn_proj_b;  /* [C][C], [C] */
  const void* head_gamma;                 /* encoder.head.0.gamma */
  sf_vae_conv head_conv;                  /* encoder.head.2 (cout = 2 z_dim) */
} sf_vae_encoder;

/* State / scratch as for the decoder, for pixel frames of H x W (multiples of 2^(n_stages-1)); `window_frames` (2..64):
 * a call encodes up to window_frames - 1 chunks of 4 pixel frames. */
size_t sf_vae_encode_state_bytes(const sf_vae_encoder* enc, int H, int W, int window_frames);
size_t sf_vae_encode_scratch_bytes(const sf_vae_encoder* enc, int H, int W, int window_frames);
/* WanVAE_.clear_cache (vae.py:610-617) of the encoder's histories. */
int sf_vae_encode_reset(const sf_vae_encoder* enc, void* state, size_t state_bytes, int H, int W, int window_frames,
                        void* stream);
/* n_chunks iterations of the chunk loop of WanVAE_.encode (vae.py:525-537) in one call: chunk_index = chunks encoded
 * into `state` since its reset; chunk 0 is ONE pixel frame encoded alone (n_chunks = 1), every later chunk 4 frames.
 * pixels: the call's frames, [3][T][H][W] with channel stride c_stride (elements; bf16, or float32 when is_f32),
 * T = 1 (chunk 0) or 4 n_chunks.  latents_out: float32 [n_chunks][z_dim][H/8][W/8], normalised mu.  `window` /
 * `history_at` place the sliding history windows exactly as for sf_vae_decode_frames.  Bit-identical to n_chunks
 * single-chunk calls. */
int sf_vae_encode_frames(const sf_vae_encoder* enc, void* state, size_t state_bytes, void* scratch, size_t scratch_bytes,
                         const void* pixels, int is_f32, int64_t c_stride, int H, int W, int window_frames,
                         int chunk_index, int n_chunks, int window, int history_at, float* latents_out, void* stream);

/* ==========================================================================================
 * TAEHV tiny decoder (latents -> pixels, the fast preview path): the demo's TAEHVDiffusersWrapper.decode ->
 * TAEHV.decode_video -> apply_model_with_memblocks over TAEHV.decoder (demo.py:60-100, demo_utils/taehv.py:60-156,
 * :181-190, :222-234).  Activations are channels-last bf16 volumes [T][H][W][C].  A MemBlock's `past` (the input of the
 * same block for the previous frame, taehv.py:33-34, :113-120) is ONE history frame kept physically in front of the new
 * frames of the block's input volume, so conv(cat[x, past]) is a causal convolution with two temporal taps.
 * ========================================================================================== */

/* The decoder's 3x3 convolution, fp32 accumulation on the matrix cores:
 *   y[(t,h,w)][n] = sum_{dt<kt,dh,dw,ci} x[t+dt][(h+dh-1)>>up][(w+dw-1)>>up][ci] * w[n][((dt*3+dh)*3+dw)*Cin + ci]
 * with zero padding in h/w.  Replaces nn.Conv2d 3x3 (taehv.py:16-17) with: the torch.cat([x, past], 1) in front of it
 * (kt = 2: tap 0 = the previous frame with weight[:, C:], tap 1 = the frame itself with weight[:, :C]; taehv.py:34), the
 * nn.ReLU behind it (taehv.py:28-31, :182, :189), a MemBlock's skip add + ReLU (taehv.py:34), nn.Upsample(scale_factor=2)
 * in front of it (taehv.py:183-188; upsample = 1), TGrow's channel -> frame re-read (taehv.py:54-57; the 1x1 convolution
 * itself is folded into w by the caller) and the demo wrapper's `* 2 - 1` with decode_to_pixel's clamp
 * (demo.py:84-89, utils/wan_wrapper.py:113). */
enum sf_taehv_epilogue {
  SF_TAEHV_BIAS_RELU = 0,        /* bf16 out = relu(y + bias)                                                    */
  SF_TAEHV_BIAS_RESID_RELU = 1,  /* bf16 out = relu(y + bias + resid[row][n])                                    */
  SF_TAEHV_PLAIN = 2,            /* bf16 out = y            (no bias read)                                       */
  SF_TAEHV_RELU = 3,             /* bf16 out = relu(y)      (no bias read)                                       */
  SF_TAEHV_HEAD_F32 = 4,         /* float out_f32[t][n][h][w] = 2 (y + bias) - 1, clamped to [-1, 1] when `clamp` */
  SF_TAEHV_LATENT_F32 = 5        /* float out_f32[t][n][h][w] = y + bias (the encoder's head, no scaling)        */
};

typedef struct sf_taehv_conv_args {
  const void* x;          /* [Tout - 1 + kt][Hin][Win][Cin], Cin % 32 == 0; kt = 2: frame 0 is the history frame  */
  const void* w;          /* [Cout][ldw]: k = tap*Cin + ci, zero padded to ldw >= roundup(kt*9*Cin, 64)           */
  const void* bias;       /* [Cout]; may be NULL for the bias-free epilogues                                      */
  void* out;              /* rows of ldo channels; row = t'*H*W + h*W + w                                         */
  const void* resid;      /* [Tout*H*W] rows of ldr channels                                                      */
  float* out_f32;         /* SF_TAEHV_HEAD_F32 / SF_TAEHV_LATENT_F32 only: [Tout][Cout][H][W], Cout <= 32         */
  int32_t Tout, H, W;     /* output frames and frame size; the input frame is (H, W), or (H/2, W/2) with upsample */
  int32_t Cin, Cout;
  int32_t kt;             /* temporal taps, 1 or 2                                                                */
  int32_t upsample;       /* 1: read the input through a nearest-neighbour 2x upsampling                          */
  int32_t ldw, ldo, ldr;
  int32_t tgrow;          /* 0 / 1: none; 2: channel n of frame t goes to frame t' = 2t + n / (Cout/2), channel
                             n % (Cout/2) (bias-free epilogues only)                                              */
  int32_t epilogue;       /* enum sf_taehv_epilogue */
  int32_t clamp;          /* SF_TAEHV_HEAD_F32: clamp to [-1, 1]                                                  */
} sf_taehv_conv_args;

int sf_taehv_conv(const sf_taehv_conv_args* args, void* stream);
int sf_taehv_pick_nt(int cout);   /* column tiles (of 16) per wave the launcher will use for Cout: 4, 2 or 1       */

/* Latent frames -> input of decoder.1: Clamp (3 tanh(z / 3) in fp32, taehv.py:20-22) and the layout change
 * [n][z][h][w] bf16 -> [n][h][w][c_pad] bf16 (channels z..c_pad-1 zero). */
int sf_taehv_prepare_latent(const void* latent, void* out, int n, int z, int h, int w, int c_pad, void* stream);

typedef struct sf_taehv_layer {
  const void* w;          /* repacked [cout][ldw] as sf_taehv_conv_args.w                                         */
  const void* bias;       /* [cout], NULL where the reference layer has none                                      */
  int32_t cin, cout, kt, ldw;   /* cin already padded to a multiple of 32                                         */
} sf_taehv_layer;

#define SF_TAEHV_STAGES 3
#define SF_TAEHV_BLOCKS 3

typedef struct sf_taehv_model {           /* TAEHV.decoder, taehv.py:181-190 (default time / space upscale)       */
  int32_t z_dim;                          /* 16 */
  sf_taehv_layer in_conv;                 /* decoder.1 (z_dim -> 256), cin padded to 32                           */
  sf_taehv_layer block[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS][3];   /* MemBlock.conv.0 (kt = 2) / .2 / .4              */
  sf_taehv_layer exit_conv[SF_TAEHV_STAGES];   /* TGrow folded into the bias-free 3x3 behind it: cout = tgrow * C' */
  int32_t tgrow[SF_TAEHV_STAGES];         /* frames per input frame at each stage exit: 1, 2, 2                   */
  sf_taehv_layer head;                    /* decoder.22 (64 -> 3)                                                 */
} sf_taehv_model;

/* Per-stream persistent state = the one-frame history of each of the nine MemBlock input volumes (channels-last bf16);
 * scratch = everything else (the volumes themselves included: a call copies the nine histories in, and its last frames
 * out), reusable by any stream that does not overlap in time.  0 = malformed arguments (sf_last_error says which). */
size_t sf_taehv_state_bytes(const sf_taehv_model* model, int lat_h, int lat_w);
size_t sf_taehv_scratch_bytes(const sf_taehv_model* model, int lat_h, int lat_w, int max_frames);
/* Zero every history: the first frame's `past` is zero (taehv.py:115-116). */
int sf_taehv_reset(const sf_taehv_model* model, void* state, size_t state_bytes, int lat_h, int lat_w, void* stream);
/* n_frames latent frames [n_frames][z][lat_h][lat_w] bf16, as the generator emits them, -> 4 n_frames pixel frames
 * [4 n_frames][3][8 lat_h][8 lat_w] float32 = decode_video(...) * 2 - 1 (demo.py:84-89), clamped to [-1, 1] when `clamp`.
 * Nothing is trimmed: the caller drops the first 3 frames after a reset (demo.py:432-433).  Bit-identical to n_frames
 * single-frame calls.  The library keeps no state of its own. */
int sf_taehv_decode_frames(const sf_taehv_model* model, void* state, size_t state_bytes, void* scratch,
                           size_t scratch_bytes, const void* latent_frames, int lat_h, int lat_w, int n_frames,
                           int clamp, float* pixels_out, void* stream);

/* ==========================================================================================
 * TAEHV tiny encoder (pixels -> latents): TAEHV.encode_video -> apply_model_with_memblocks over TAEHV.encoder
 * (demo_utils/taehv.py:172-178, :210-220).  Four pixel frames make one latent frame at 1/8 of the size.  The volumes
 * and the MemBlock histories are the decoder's; TPool (taehv.py:37-45) never runs as a layer: it is folded by the caller
 * into the bias-free stride-2 convolution behind it, which then has kt = TPool's stride temporal taps and that temporal
 * stride (taehv_weights.fold_tpool).
 * ========================================================================================== */

enum sf_taehv_pixel_dtype { SF_TAEHV_PIXEL_BF16 = 0, SF_TAEHV_PIXEL_F32 = 1 };

/* encoder.0 + ReLU at full resolution, straight from the caller's pixels:
 *   out[t][h][w][n] = relu(bias[n] + sum_{dh,dw,c} u[src(t)][h+dh-1][w+dw-1][c] * w[n][(dh*3+dw)*3 + c]),
 *   u = bf16(0.5 * pixel + 0.5) inside the image and 0 outside, src(t) = max(t - lead, 0).
 * pixels: [3][n_frames - lead][H][W] with channel stride c_stride (elements), values in [-1, 1], bf16 or float32.
 * w: bf16 [64][32], k = (dh*3+dw)*3 + c, columns 27..31 zero; bias bf16 [64]; out: channels-last bf16
 * [n_frames][H][W][64].  lead in 0..3 and below n_frames. */
int sf_taehv_encode_stem(const void* pixels, int dtype, int64_t c_stride, int H, int W, int n_frames, int lead,
                         const void* w, const void* bias, void* out, void* stream);

/* The encoder's strided convolution (TPool folded in), bf16 out, no bias:
 *   y[(t,h,w)][n] = sum_{dt<kt,dh,dw,ci} x[kt*t + dt][2h+dh-1][2w+dw-1][ci] * w[n][((dt*3+dh)*3+dw)*Cin + ci]
 * with zero padding in h/w: kt temporal taps at temporal stride kt, spatial stride 2.  The shared implicit-GEMM core of
 * sf_taehv_conv with compile-time strides. */
typedef struct sf_taehv_down_conv_args {
  const void* x;          /* [kt*Tout][2H][2W][Cin], Cin % 32 == 0                                                */
  const void* w;          /* [Cout][ldw] as sf_taehv_conv_args.w                                                  */
  void* out;              /* rows of ldo channels; row = t*H*W + h*W + w                                          */
  int32_t Tout, H, W;     /* output frames and frame size; the input frame is (2H, 2W)                            */
  int32_t Cin, Cout;      /* Cout % 64 == 0                                                                       */
  int32_t kt;             /* temporal taps = temporal stride, 1 or 2                                              */
  int32_t ldw, ldo;
} sf_taehv_down_conv_args;

int sf_taehv_down_conv(const sf_taehv_down_conv_args* args, void* stream);

typedef struct sf_taehv_encoder {         /* TAEHV.encoder, taehv.py:172-178                                      */
  sf_taehv_layer stem;                    /* encoder.0 (3 -> 64) as sf_taehv_encode_stem reads it: cin = ldw = 32 */
  sf_taehv_layer down[SF_TAEHV_STAGES];   /* TPool folded into the stride-2 3x3 behind it: kt = 2, 2, 1           */
  sf_taehv_layer block[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS][3];   /* MemBlock.conv.0 (kt = 2) / .2 / .4              */
  sf_taehv_layer head;                    /* encoder.17 (64 -> z_dim = head.cout)                                 */
} sf_taehv_encoder;

/* Per-stream persistent state = the one-frame history of each of the nine MemBlock input volumes (at 1/2, 1/4 and 1/8
 * of H x W); a call carries whole groups of four pixel frames, so TPool holds nothing between calls.  scratch =
 * everything else, for calls of up to max_frames pixel frames.  0 = malformed arguments (sf_last_error says which). */
size_t sf_taehv_encode_state_bytes(const sf_taehv_encoder* enc, int H, int W);
size_t sf_taehv_encode_scratch_bytes(const sf_taehv_encoder* enc, int H, int W, int max_frames);
/* Zero every history: the first frame's `past` is zero (taehv.py:115-116). */
int sf_taehv_encode_reset(const sf_taehv_encoder* enc, void* state, size_t state_bytes, int H, int W, void* stream);
/* n_frames frames (a multiple of 4; H, W multiples of 8), frame t being pixel frame max(t - lead, 0) of `pixels`
 * ([3][n_frames - lead][H][W] with channel stride c_stride, enum sf_taehv_pixel_dtype, values in [-1, 1]) ->
 * n_frames / 4 latent frames float32 [n_frames / 4][z_dim][H/8][W/8] = encode_video((pixels + 1) / 2), in the
 * generator's space (no mean / std).  Bit-identical however a clip is cut into calls.  The library keeps no state. */
int sf_taehv_encode_frames(const sf_taehv_encoder* enc, void* state, size_t state_bytes, void* scratch,
                           size_t scratch_bytes, const void* pixels, int dtype, int64_t c_stride, int H, int W,
                           int n_frames, int lead, float* latents_out, void* stream);

/* ==========================================================================================
 * JPEG encoder (decoded frames -> JFIF files): what the demo's sender does on the host (demo.py:162-187: clamp, * 127.5
 * + 127.5, truncate to uint8, PIL save) as three kernels, so that a frame leaves the GPU as 0.1-0.4 MB of JPEG instead
 * of 4.8 MB of fp32.  Baseline sequential JFIF, 8 bit, Y Cb Cr (JFIF's full-range BT.601), 4:2:0 (chroma = the 2x2 mean)
 * or 4:4:4, libjpeg's quality scaling of the Annex K tables, the Annex K Huffman tables, a DRI segment and RST0..7
 * every `restart_interval` MCUs (one wave codes one interval).  h and w must be multiples of the MCU (16 for 4:2:0, 8
 * for 4:4:4).  The numbers are defined by self_forcing_amd/jpeg_reference.py; the library keeps no state and uploads
 * nothing (tables and the header travel as kernel arguments).
 * ========================================================================================== */

enum sf_jpeg_subsampling { SF_JPEG_420 = 0, SF_JPEG_444 = 1 };
enum sf_jpeg_dtype { SF_JPEG_U8 = 0, SF_JPEG_F32 = 1, SF_JPEG_BF16 = 2 };   /* u8: [n][h][w][3]; f32 / bf16: planar [n][3][h][w] */
enum sf_jpeg_range {
  SF_JPEG_RANGE_PM1 = 0,   /* u8 = trunc(clamp(p, -1, 1) * 127.5 + 127.5), each operation rounded to fp32 (demo.py:166-167) */
  SF_JPEG_RANGE_01 = 1     /* u8 = trunc(255 * clamp(x, 0, 1))                                                            */
};
/* bits the kernels OR into *status (0 = every file is complete) */
enum sf_jpeg_status {
  SF_JPEG_SLOT_OVERFLOW = 1,   /* an interval outgrew its worst-case slot (cannot happen for coefficients in range)       */
  SF_JPEG_COEF_RANGE = 2,      /* a DC difference beyond category 11 or an AC coefficient beyond category 10              */
  SF_JPEG_OUT_OVERFLOW = 4     /* the files need more than out_capacity bytes: offsets are valid, nothing was written     */
};

/* Bytes of workspace for n frames: the coefficient buffer (int16 [n][blocks][64], at the start), one slot per restart
 * interval sized for its worst case (1660 bits per block, every byte stuffed), and the interval lengths and positions.
 * 0 = malformed arguments (sf_last_error says which). */
size_t sf_jpeg_workspace_bytes(int n, int h, int w, int subsampling, int restart_interval);
/* frames -> quantised coefficients, zigzagged, int16 [n][blocks][64] in MCU scan order (Y00 Y01 Y10 Y11 Cb Cr per 16x16 MCU
 * for 4:2:0, Y Cb Cr per 8x8 MCU for 4:4:4): truncation to 8 bit in fp32 (enum sf_jpeg_range), then colour conversion,
 * chroma mean, 8x8 DCT and q = rint(c / Q) in fp64.  bf16 frames are widened to fp32 first.  value_range is ignored
 * for SF_JPEG_U8. */
int sf_jpeg_transform(const void* frames, int dtype, int value_range, int n, int h, int w, int subsampling, int quality,
                      void* coef, void* stream);
/* coefficients -> n whole files back to back in `out`; file f is out[offsets[f] .. offsets[f + 1]).  `workspace` as sized
 * by sf_jpeg_workspace_bytes (its coefficient part is not touched unless `coef` points at it); offsets int64 [n + 1],
 * status int32 [1] (enum sf_jpeg_status bits), both device memory written on `stream`.  out_capacity =
 * sf_jpeg_workspace_bytes(...) always suffices. */
int sf_jpeg_entropy(const void* coef, int n, int h, int w, int subsampling, int quality, int restart_interval,
                    void* workspace, size_t workspace_bytes, void* out, size_t out_capacity, int64_t* offsets,
                    int32_t* status, void* stream);
/* Both steps for a group of frames in one host call. */
int sf_jpeg_encode_frames(const void* frames, int dtype, int value_range, int n, int h, int w, int subsampling,
                          int quality, int restart_interval, void* workspace, size_t workspace_bytes, void* out,
                          size_t out_capacity, int64_t* offsets, int32_t* status, void* stream);

/* ==========================================================================================
 * JPEG decoder (JFIF files -> pixels): the way back in, for pose frames that arrive as JPEG (a renderer behind a socket,
 * a webcam, an MJPEG file this project wrote).  Baseline sequential DCT, 8 bit, Huffman, one interleaved scan; Y Cb Cr
 * with luma sampling 2x2 / 1x1 / 2x1 over 1x1 chroma, or one component; any tables, with or without DRI, any h, w >= 1
 * (the padding blocks are decoded and cropped).  Four kernels: restart-marker search, entropy decoding (one lane per
 * restart interval), dequantisation + IDCT, chroma upsampling + colour + output format.  All arithmetic is integer and
 * exact: X = coef Q, t = Bi^T X Bi with Bi[k][n] = rint(2^13 b(k, n)) in 64 bits, sample = clamp(((t + 2^25) >> 26) + 128),
 * libjpeg's "fancy" triangle filter for the chroma, 16.16 fixed point for the colour matrix.  The numbers are defined by
 * self_forcing_amd/jpeg_reference.py (`decode`), which the kernels equal bit for bit.
 *
 * The caller reads the files' header segments on the host (the library never parses a file) and uploads ONE buffer:
 * n table entries of SF_JPEG_DECODE_FILE_BYTES each, then the files' bytes.  A table entry (little endian):
 *   uint32 scan_off, scan_len     the entropy-coded bytes of the file: upload[scan_off .. scan_off + scan_len)
 *   uint32 ri, intervals          MCUs per restart interval (the MCU count without DRI), ceil(MCUs / ri)
 *   uint16 quant[3][64]           per component, natural order
 *   huff[3][2]                    per component DC, AC: uint16 look[512] ((length << 8) | symbol of the code the next 9
 *                                 bits start with, 0 = longer), int32 maxcode[18], int32 valoff[18] (T.81 F.2.2.3:
 *                                 symbol = vals[code + valoff[L]] for the first L with code <= maxcode[L]), uint8 vals[256]
 *   16 bytes of padding
 * The kernels trust nothing in it: reads are clamped to the upload, writes to the call's geometry.  A file without DRI
 * is one interval, so one lane decodes all of it: correct, and slow.
 * ========================================================================================== */

#define SF_JPEG_DECODE_FILE_BYTES 8960
/* (the first two as enum sf_jpeg_subsampling) */
enum sf_jpeg_decode_sampling { SF_JPEG_DEC_420 = 0, SF_JPEG_DEC_444 = 1, SF_JPEG_DEC_422 = 2, SF_JPEG_DEC_GRAY = 3 };
/* with enum sf_jpeg_dtype: u8 = the decoded samples; f32 / bf16 = u8 / 127.5 - 1, the divide and the subtract each
 * rounded to fp32, bf16 by round-to-nearest-even */
enum sf_jpeg_layout {
  SF_JPEG_HWC = 0,    /* [n][h][w][3]: what the encoder takes as SF_JPEG_U8    */
  SF_JPEG_POSE = 1,   /* [3][n][h][w]: what sf_pose_embed takes                */
  SF_JPEG_CHW = 2     /* [n][3][h][w]: what the VAE encoders take              */
};
/* bits the kernels OR into status[file] (0 = the file decoded completely) */
enum sf_jpeg_decode_status {
  SF_JPEG_DEC_BAD_CODE = 1,       /* a bit pattern that is no Huffman code, or a DC category beyond 11                  */
  SF_JPEG_DEC_RUN_PAST_63 = 2,    /* a zero run that ends behind the 63rd coefficient                                   */
  SF_JPEG_DEC_TRUNCATED = 4,      /* a restart interval ended before its blocks did                                     */
  SF_JPEG_DEC_MARKER_COUNT = 8    /* the scan holds another number of RSTn markers than intervals - 1                   */
};

/* Workspace for n files of h x w: the coefficients, the component planes, the marker table.  max_intervals = the
 * largest `intervals` of the call's table entries.  0 = malformed arguments (sf_last_error says which). */
size_t sf_jpeg_decode_workspace_bytes(int n, int h, int w, int sampling, int max_intervals);
/* upload -> coef int16 [n][blocks][64]: quantised coefficients, zigzagged, in MCU scan order, the padding MCUs included
 * (Y00 Y01 Y10 Y11 Cb Cr for 4:2:0, Y Cb Cr for 4:4:4, Y0 Y1 Cb Cr for 4:2:2, raster 8x8 blocks for grayscale).  status
 * int32 [n], device memory written on `stream`.  `coef` may be the workspace's own (offset 0). */
int sf_jpeg_decode_entropy(const void* upload, size_t upload_bytes, int n, int h, int w, int sampling, int max_intervals,
                           void* workspace, size_t workspace_bytes, void* coef, int32_t* status, void* stream);
/* coef -> out in `layout` / `dtype`.  idct_table: HOST int32 [64], Bi[k * 8 + n] = rint(2^13 b(k, n)) (the caller computes
 * it, so the kernels and their definition share one source). */
int sf_jpeg_decode_pixels(const void* coef, const void* upload, size_t upload_bytes, const int32_t* idct_table, int n,
                          int h, int w, int sampling, void* workspace, size_t workspace_bytes, void* out, int layout,
                          int dtype, void* stream);
/* Both steps in one host call. */
int sf_jpeg_decode_frames(const void* upload, size_t upload_bytes, const int32_t* idct_table, int n, int h, int w,
                          int sampling, int max_intervals, void* workspace, size_t workspace_bytes, void* out, int layout,
                          int dtype, int32_t* status, void* stream);

/* ==========================================================================================
 * Frame resizer (uint8 frames -> frames of another size): what the reference does on the host with Pillow
 * (inference.py:84-88, transforms.Resize on a PIL image = antialiased bilinear; causal_diffusion_inference.py:158,
 * image.resize = bicubic), with Pillow's bits.  Pillow's 8-bit resampler is exact integer arithmetic: per axis a table of
 * 22-bit fixed-point coefficients, one pass
 *   out = clamp((2^21 + sum_{x < xmax} px[xmin + x] * coef[x]) >> 22, 0, 255)      (arithmetic shift, int32)
 * the horizontal pass first, rounded to uint8, then the vertical pass over its result.  The numbers are defined by
 * self_forcing_amd/resize_reference.py (`coefficients`, `resize`), which the kernel equals bit for bit.
 *
 * The caller computes the two tables (the library never does: the double-precision arithmetic has one definition) and
 * passes them as DEVICE memory, for an axis of `in` pixels (the crop's size) resampled to `out`:
 *   bounds int32 [out][2]    (xmin, xmax): the first input pixel and the number of taps of output pixel xx, relative to
 *                            the crop; 0 <= xmin, xmin + xmax <= in, xmax <= ks
 *   coefs  int32 [out][ks]   ks = sf_resize_kernel_size(in, out, filter) = ceil(support * max(in / out, 1)) * 2 + 1 with
 *                            support 1 (bilinear) or 2 (bicubic); entries past xmax are not read
 * An axis that keeps its size takes the table the same arithmetic gives (one weight 1 << 22): no special case.  The
 * kernel clamps what it reads from the tables to the crop, so a wrong table gives wrong pixels and nothing else.
 * One fused kernel (a workgroup resamples the input rows of a 16 x 64 output tile horizontally into LDS, then that
 * vertically); its LDS grows with the reduction, so in / out may be at most SF_RESIZE_MAX_RATIO per axis (any
 * enlargement is taken); a larger reduction is refused.  The library keeps no state and needs no workspace.
 * ========================================================================================== */

#define SF_RESIZE_MAX_RATIO 8
enum sf_resize_filter { SF_RESIZE_BILINEAR = 0, SF_RESIZE_BICUBIC = 1 };

/* Columns of the coefficient table of one axis; 0 = malformed arguments (sf_last_error says which). */
int sf_resize_kernel_size(int in_size, int out_size, int filter);
/* frames uint8 in `layout` (enum sf_jpeg_layout, n frames of h x w) -> out in `out_layout` / `out_dtype` (enum
 * sf_jpeg_dtype: u8 = the samples, f32 / bf16 = u8 / 127.5 - 1 as the decoder converts), n frames of out_h x out_w.
 * crop: HOST int32 [4] = (top, left, height, width) inside the frame, or NULL for the whole frame: exactly
 * im.crop(...).resize(...), no tap reaches outside it.  The tables are for crop size -> output size.  frames 4-byte, out
 * 16-byte aligned. */
int sf_resize_frames(const void* frames, int layout, int n, int h, int w, const int32_t* crop, const int32_t* bounds_h,
                     const int32_t* coefs_h, const int32_t* bounds_v, const int32_t* coefs_v, int filter, void* out,
                     int out_layout, int out_dtype, int out_h, int out_w, void* stream);

/* ==========================================================================================
 * Raw YUV frames <-> RGB frames: the pixel formats of video outside JPEG (a V4L2 webcam's YUYV, a hardware codec's NV12,
 * the I420 / I422 / I444 planes and YUV4MPEG2 streams of software tools).  The reference takes its frames through PIL / cv2
 * on the host (inference.py:84-88 and the pose loaders) and uploads RGB; here 1.5 or 2 bytes per pixel cross the bus and
 * the conversion runs on the device.  8 bit, tightly packed, ch = ceil(h / 2), cw = ceil(w / 2):
 *   I420  Y [h][w], U [ch][cw], V [ch][cw]        NV12  Y [h][w], UV [ch][cw][2]
 *   I422  Y [h][w], U [h][cw], V [h][cw]          I444  Y, U, V [h][w] each
 *   GRAY  Y [h][w] (U = V = 128)                  YUYV  [h][w / 2][4] = Y0 U Y1 V      UYVY  = U Y0 V Y1   (w even)
 * The encoder writes the first four.  A frame's size may be odd, so frame k of a batch may start at any byte.
 *
 * constants: HOST int32 [16] = (yoff, CY, CRV, CGU, CGV, CBU, YR, YG, YB, UR, UG, UB, VR, VG, VB, 0), computed by the
 * caller with self_forcing_amd/yuv_reference.py `constants(matrix, range)` (BT.601 / BT.709, full / limited range, 16-bit
 * fixed point): the library holds no colour matrix of its own.  All arithmetic int32, shifts arithmetic, clamp to 0..255:
 *   y = (Y - yoff) CY     cb = U - 128     cr = V - 128
 *   R = clamp((y + CRV cr + 32768) >> 16)     G = clamp((y - CGU cb - CGV cr + 32768) >> 16)     B = clamp((y + CBU cb + 32768) >> 16)
 *   Y = clamp(( YR R + YG G + YB B + (yoff << 16) + 32768) >> 16)
 *   U = clamp((-UR R - UG G + UB B + (128 << 16) + 32767) >> 16)     V = clamp((VR R - VG G - VB B + (128 << 16) + 32767) >> 16)
 * Subsampled chroma is up-sampled by replication (NEAREST) or by libjpeg's triangle filter for centre-sited chroma
 * (TRIANGLE: the JPEG decoder's, edges replicated); the encoder converts every pixel and averages 2 x 2 as
 * (a + b + c + d + 2) >> 2 and 2 x 1 as (a + b + 1) >> 1, an odd size's missing column or row being the edge's again.
 * For BT.601 full range the decode is the JPEG decoder's colour step bit for bit.  One launch per call for all frames;
 * the library keeps no state and needs no workspace.
 * ========================================================================================== */

#define SF_YUV_MAX_SIZE 16384
enum sf_yuv_format {
  SF_YUV_I420 = 0, SF_YUV_NV12 = 1, SF_YUV_I422 = 2, SF_YUV_I444 = 3,   /* decode and encode */
  SF_YUV_GRAY = 4, SF_YUV_YUYV = 5, SF_YUV_UYVY = 6                     /* decode only       */
};
enum sf_yuv_chroma { SF_YUV_NEAREST = 0, SF_YUV_TRIANGLE = 1 };

/* Bytes of one h x w frame; 0 = malformed arguments (sf_last_error says which). */
size_t sf_yuv_frame_bytes(int format, int h, int w);
/* raw: n frames back to back (any alignment) -> out in `layout` / `dtype` (enum sf_jpeg_layout / sf_jpeg_dtype: u8 = the
 * samples, f32 / bf16 = u8 / 127.5 - 1 as the JPEG decoder converts), 16-byte aligned. */
int sf_yuv_decode_frames(const void* raw, int format, int n, int h, int w, const int32_t* constants, int chroma,
                         void* out, int layout, int dtype, void* stream);
/* frames: u8 [n][h][w][3], or f32 / bf16 [n][3][h][w] in `value_range` (enum sf_jpeg_range, truncated to 8 bit as the JPEG
 * encoder does) -> out: n frames of `format` back to back. */
int sf_yuv_encode_frames(const void* frames, int dtype, int value_range, int n, int h, int w, const int32_t* constants,
                         void* out, int format, void* stream);

/* ==========================================================================================
 * Pose renderer (DWPose whole-body keypoints -> skeleton frames).  The reference has no renderer: its dwpose_data
 * arrives already drawn, in the DWPose style of UniAnimate-DiT.  The drawing is this project's definition in that style,
 * self_forcing_amd/pose_render_reference.py (`quantize`, `primitives`, `inside`), in exact integer arithmetic; the kernel
 * equals it bit for bit.  Per person 185 primitives in a fixed painter's order: 17 limbs (ellipses with semi-axes
 * (length / 2, 4), in 3/5 of the palette colour), 18 body joints (discs, r = 4), per hand 20 edges (capsules of
 * half-width 1) and 21 discs (r = 4), 68 face discs (r = 3).
 *   keypoints float32 [F][P][134][3] = (x, y, score), DWPose's order: 0-17 body, 18-23 feet (ignored), 24-91 face,
 *             92-112 left hand, 113-133 right hand
 *   pixel     normalized: X = (int)(x * W), Y = (int)(y * H), one fp32 multiply; else X = (int)x, Y = (int)y
 *   valid     x, y, score finite, score >= score_threshold, x >= 0, y >= 0, X and Y <= SF_POSE_RENDER_MAX_COORD
 * One kernel, one launch for all frames: a workgroup per 16 x 64 tile lists the primitives whose box reaches the tile
 * in LDS, then every lane decides four pixels from the back of the list.  The library keeps no state and needs no
 * workspace.
 * ========================================================================================== */

#define SF_POSE_RENDER_MAX_PEOPLE 8
#define SF_POSE_RENDER_MAX_SIZE 4096
#define SF_POSE_RENDER_MAX_COORD 8191

typedef struct sf_pose_render_args {
  const float* keypoints;     /* DEVICE float32 [F][P][134][3], 4-byte aligned                                     */
  void* out;                  /* F frames of H x W in `layout` / `dtype`, 16-byte aligned; every element is written */
  int32_t F, P, H, W;         /* 1 <= F <= 65535, 1 <= P <= SF_POSE_RENDER_MAX_PEOPLE, 1 <= H, W <= SF_POSE_RENDER_MAX_SIZE */
  int32_t layout;             /* enum sf_jpeg_layout                                                               */
  int32_t dtype;              /* enum sf_jpeg_dtype: u8 = the samples, f32 / bf16 = u8 / 127.5 - 1 as the decoder converts */
  int32_t normalized;         /* 1: x, y in [0, 1]; 0: in pixels                                                   */
  float score_threshold;      /* finite; DWPose's drawing uses 0.3                                                 */
} sf_pose_render_args;

int sf_pose_render_frames(const sf_pose_render_args* args, void* stream);

/* ==========================================================================================
 * Pose retargeter (driving keypoints -> keypoints of the reference person's proportions, on the generator's timeline).
 * The reference has no counterpart: its poses arrive drawn and aligned.  The numbers are this project's definition,
 * self_forcing_amd/pose_retarget_reference.py (`lift`, `resample`, `fit`, `retarget_frame`): float32, every sub, mul,
 * add, div and sqrt rounded on its own; the kernel equals it bit for bit.
 *   valid     the renderer's rule on the raw values: x, y, score finite, score >= score_threshold, x >= 0, y >= 0;
 *             an invalid output point is (-1, -1, 0)
 *   lift      x * sx, y * sy, one fp32 multiply each; the factors come from the host (formed in double, rounded once)
 *   resample  output frame j sits at source position j * num / den: i0 = j num / den, rem = j num % den, i1 = i0 + (rem != 0);
 *             rem == 0 copies; both valid: a + (rem / den) * (b - a), score the smaller; one valid: taken when nearer
 *             (a when 2 rem <= den)
 *   fit       per person from clip frame 0 and the reference over the renderer's 17 limbs: a global ratio g of summed
 *             lengths, nine ratios of symmetric limb groups; the anchor is the neck (point 1), without it in both the
 *             person is lifted and resampled only
 *   retarget  the neck goes to R[1] + g * (q - S0[1]); every other point is placed from its parent (limbs) or anchor
 *             (feet, face, hands) at ratio * its offset in the resampled frame
 * One kernel, one launch per piece, a workgroup per (output frame, person).  The library keeps no state and needs no
 * workspace; a streaming caller keeps clip frame 0 and the last source frame it has seen.
 * ========================================================================================== */

#define SF_POSE_RETARGET_MAX_RATE 65535
#define SF_POSE_RETARGET_MAX_FRAMES 1048576

typedef struct sf_pose_retarget_args {
  const float* src;           /* DEVICE float32 [n_src][people][134][3]: clip frames src0 .. src0 + n_src - 1          */
  const float* first;         /* DEVICE float32 [people][134][3]: clip frame 0 (S0), as it came                        */
  const float* ref;           /* DEVICE float32 [ref_people][134][3]                                                   */
  float* out;                 /* DEVICE float32 [n_out][people][134][3]: output frames out0 ..; every element is written */
  int64_t src0;               /* clip index of src's first frame                                                       */
  int64_t out0;               /* index of the first output frame                                                       */
  int32_t n_src, n_out;       /* n_src >= 1, 1 <= n_out <= SF_POSE_RETARGET_MAX_FRAMES; i0 and i1 of every output frame lie in src */
  int32_t people, ref_people; /* 1 <= people <= SF_POSE_RENDER_MAX_PEOPLE; ref_people = 1 (serves everyone) or people  */
  int32_t num, den;           /* source_fps / target_fps in lowest terms, both 1 .. SF_POSE_RETARGET_MAX_RATE          */
  float src_sx, src_sy;       /* lift of the source, finite                                                            */
  float ref_sx, ref_sy;       /* lift of the reference, finite                                                         */
  float score_threshold;      /* finite                                                                                */
  int32_t align;              /* 1: fit and retarget; 0: lift and resample only                                        */
} sf_pose_retarget_args;

int sf_pose_retarget_frames(const sf_pose_retarget_args* args, void* stream);

/* Host only: the output frames that become final once n more source frames follow the `frames_before` already seen
 * (frame j is final when source frame i1(j) is in): [*first_out, *first_out + *n_out).  A clip of F frames gives
 * (F - 1) * den / num + 1 output frames. */
int sf_pose_retarget_plan(int64_t frames_before, int64_t n, int num, int den, int64_t* first_out, int64_t* n_out);

/* ==========================================================================================
 * Pose smoother (jittery keypoints with dropped points -> smoothed keypoints, in front of the retargeter).  The reference
 * has no counterpart: its poses arrive drawn.  The numbers are this project's definition,
 * self_forcing_amd/pose_smooth_reference.py (`frames`): a One-Euro filter per point on x and y with a bounded hold across
 * missing samples, float32, every sub, mul, add and div rounded on its own; the kernel equals it bit for bit.
 *   valid     the renderer's rule on the raw values: x, y, score finite, score >= score_threshold, x >= 0, y >= 0
 *   state     per (person, point) 8 words of 32 bits: hx, hy (filtered position), dx, dy (filtered speed), s (the last
 *             valid score) as float; gap (frames since the last valid sample), seen as int32; 0.  Zero-filled is fresh.
 *   a frame   te = (float)(gap + 1) * period.
 *             valid and seen: per coordinate with sample v:  e = v - h;  dx = e / te;  rd = kd * te;  ad = rd / (rd + 1);
 *               t = dx - d;  t = ad * t;  d' = d + t;  fc = beta * |d'|;  fc = min_cutoff + fc;  r = fp32(2 pi) * fc;
 *               r = r * te;  a = r / (r + 1);  t = a * e;  h' = h + t.  All four of h', d' finite: they become the state;
 *               else the point is seeded afresh.
 *             valid and not seen, or seeded afresh: h = (x, y), d = 0.
 *             either valid case: s = score, gap = 0, seen = 1; the output is (hx, hy, s).
 *             invalid, seen and gap < max_gap: gap += 1; the output is (hx, hy, s).
 *             invalid otherwise: seen = 0, gap = 0; the output is (-1, -1, 0); h, d and s keep their bits.
 * One kernel, one launch per piece, one lane per (person, point) that walks the piece's frames with its state in
 * registers.  The library keeps no state and needs no workspace: the caller owns `state` and hands it to every piece of
 * one clip, so any partition of a clip gives the whole clip's bits.
 * ========================================================================================== */

typedef struct sf_pose_smooth_args {
  const float* src;           /* DEVICE float32 [n][people][134][3], in the caller's units                             */
  float* out;                 /* DEVICE float32 [n][people][134][3]; every element is written                          */
  void* state;                /* DEVICE [people][134][8] 32-bit words, 16-byte aligned; read and advanced              */
  int32_t n, people;          /* 1 <= n <= SF_POSE_RETARGET_MAX_FRAMES, 1 <= people <= SF_POSE_RENDER_MAX_PEOPLE; src, out and state do not overlap */
  float period;               /* seconds per frame, fp32(den / num) of the source rate; finite, > 0                    */
  float min_cutoff;           /* Hz; finite, > 0                                                                       */
  float beta;                 /* 1 / unit; finite, >= 0                                                                */
  float kd;                   /* fp32(2 pi d_cutoff); finite, > 0                                                      */
  float score_threshold;      /* finite                                                                                */
  int32_t max_gap;            /* 0 .. 65535: the longest run of invalid samples that is bridged                        */
} sf_pose_smooth_args;

int sf_pose_smooth_frames(const sf_pose_smooth_args* args, void* stream);

/* Host only: the bytes of `state` for `people` people (people * 134 * 32); 0 for people out of range. */
size_t sf_pose_smooth_state_bytes(int people);

/* ==========================================================================================
 * Pose tracker (the people of each frame in the detector's order -> each person in one stable slot, in front of the
 * smoother).  The reference has no counterpart: its poses arrive drawn.  The numbers are this project's definition,
 * self_forcing_amd/pose_track_reference.py (`frames`): float32, every sub, mul, add and div rounded on its own; the
 * kernels equal it bit for bit.  A slot's output row is the matched detection's 134 x 3 floats copied bit for bit, or
 * the marker (-1, -1, 0) at all 134 points; ids[f][s] is the track id, -1 beside a marker row.
 *   valid     a point, by the renderer's rule on the raw values: x, y, score finite, score >= score_threshold, x >= 0,
 *             y >= 0.  Only the body points 0..17 are matched; a detection is a person iff >= min_points of them are valid.
 *   state     [slots + 1][40] 32-bit words.  Row s < slots: words 0..35 the float bits of x, y of the 18 points of the
 *             last detection matched to the slot, 36 their validity mask (bit j for point j), 37 age (frames since that
 *             match), 38 id, 39 alive.  Row `slots`: next_id in word 0, the rest is not touched.  Zero-filled is fresh.
 *   cost      of (live slot t, person d) over the points j = 0..17, ascending, valid in both (n of them):
 *               dx = xd - xt;  dy = yd - yt;  q = dx * dx + dy * dy;  acc = acc + q;
 *             w, h = max - min of the slot's valid x and y;  s2 = w * w + h * h;  cost = (acc / (float)n) / s2.
 *             Admissible iff n >= min_common, s2 > 0 and finite, cost finite, cost <= gate2.
 *   a frame   match: repeatedly the admissible pair of an unassigned slot and an unassigned person with the smallest
 *             (cost bits, t, d); age: a matched slot gets age = 0, an unmatched live one age += 1 and dies if
 *             age > max_age; birth: the unassigned persons in ascending order take the lowest slots that were free at the
 *             START of the frame, id = next_id++ & 0x7fffffff, and those without a slot are dropped; the memory of every
 *             slot that has a detection is replaced.
 * Two kernels on one stream: a one-wave assignment kernel that walks the piece's frames (lane = 8 * slot + detection,
 * the state in LDS) and writes assign[f][s] = the detection index or -1, and a gather kernel over every element of out.
 * The library keeps no state: the caller owns `state` and hands it to every piece of one clip, so any partition of a
 * clip gives the whole clip's bits.  `assign` is scratch of n * slots * 4 bytes; its contents after the call are the
 * detection indices.
 * ========================================================================================== */

typedef struct sf_pose_track_args {
  const float* src;           /* DEVICE float32 [n][people][134][3], in the caller's units                             */
  float* out;                 /* DEVICE float32 [n][slots][134][3]; every element is written                           */
  int32_t* ids;               /* DEVICE int32 [n][slots]; every element is written                                     */
  void* state;                /* DEVICE [slots + 1][40] 32-bit words, 16-byte aligned; read and advanced               */
  int32_t* assign;            /* DEVICE scratch int32 [n][slots], 4-byte aligned; every element is written             */
  int32_t n, people, slots;   /* 1 <= n <= SF_POSE_RETARGET_MAX_FRAMES, 1 <= people, slots <= SF_POSE_RENDER_MAX_PEOPLE; no two of the five ranges overlap */
  int32_t min_points;         /* 1 .. 18: the valid body points that make a detection a person                         */
  int32_t min_common;         /* 1 .. 18: the points a slot and a person must share to be compared                     */
  int32_t max_age;            /* 0 .. 65535: the frames a slot waits for its person before it is freed                 */
  float gate2;                /* fp32(gate * gate): the largest admissible cost; finite, > 0                           */
  float score_threshold;      /* finite                                                                                */
} sf_pose_track_args;

int sf_pose_track_frames(const sf_pose_track_args* args, void* stream);

/* Host only: the bytes of `state` for `slots` slots ((slots + 1) * 160); 0 for slots out of range. */
size_t sf_pose_track_state_bytes(int slots);

/* ==========================================================================================
 * DWPose glue (a frame on the device -> keypoints [F][P][134][3] on the device, around the caller's two networks): what
 * DWPose does in numpy and OpenCV on the host, one frame and one person at a time.  The reference has no counterpart: its
 * poses arrive drawn.  The numbers are this project's definition, self_forcing_amd/pose_estimate_reference.py
 * (`decode_boxes`, `person_window`, `crop_people`, `decode_simcc`): DWPose's formulas in float32, every add, sub, mul and
 * div rounded on its own, not OpenCV's fixed-point bits; the kernels equal it bit for bit.  DWPose's constants (640 x 640,
 * strides 8 / 16 / 32, 0.3, 0.45, 1.25, 384 x 288, split ratio 2, mean / std, the reorder) are the caller's arguments.
 *   boxes     head float32 [F][A][5 + C], anchors stride-major, then row-major (gy, gx).  cx = (o0 + gx) * s, cy likewise,
 *             w = exp32(o2) * s, h likewise (decoded: o0..o3 as they are); corners cx -+ w * 0.5 and cy -+ h * 0.5, each
 *             divided by ratio; score = o4 * o[5 + class_index].  exp32: x clamped to [-20, 20], n = rint(x * log2e), a
 *             two-constant Cody-Waite reduction, a degree-6 Taylor polynomial by Horner, ldexp; within 2^-20 of e^x.  A
 *             candidate has a finite score > score_threshold and finite corners.  Greedy NMS, at most P rounds: the largest
 *             live score (ties: the lowest anchor) is emitted and removed with every live candidate whose iou with it is
 *             > iou_threshold; area = (x2 - x1 + 1) * (y2 - y1 + 1), iw = max(0, min(x2a, x2b) - max(x1a, x1b) + 1).
 *   window    cx = (x1 + x2) * 0.5; bw = (x2 - x1) * padding; aspect = (float)out_w / (float)out_h; bw > bh * aspect ?
 *             bh = bw / aspect : bw = bh * aspect; ax = bw / out_w; ay = bh / out_h.  Valid iff all six are finite and
 *             bw, bh > 0.  A person is PRESENT iff p < count[f] and the window of boxes[f][p] is valid.
 *   crops     element (c, j, i) of a present person: sx = cx + (i - out_w * 0.5) * ax, x0 = floor(sx), fx = sx - x0 (y
 *             likewise), four taps (0 outside the frame) blended a = p00 + (p01 - p00) * fx, b likewise, v = a + (b - a) * fy,
 *             out = (v - mean[c]) / std[c]; v = 0 without a read unless -1 <= sx <= W and -1 <= sy <= H.  Other rows are 0.
 *   keypoints per (person, point) the first index of the maximum of the non-NaN entries of its simcc_x and simcc_y row;
 *             s = the smaller maximum; valid iff the person is present, s finite and > 0; x = cx + (ix / split_ratio -
 *             out_w * 0.5) * ax, y likewise, divided by W and H when normalized; else (-1, -1, 0).  The neck is the mean of
 *             COCO points 5 and 6 with score 1 when both are valid with s > neck_threshold.  tmp = 17 body points, the
 *             neck, the other 116; out[i] = tmp[order[i]].
 * Four kernels: a lane per (frame, anchor) writes the live score and the corners to `scratch`, one workgroup per frame
 * runs the NMS rounds with its live scores in registers; a lane per crop pixel; a workgroup per person for the keypoints.
 * The library keeps no state, makes no host read and no synchronisation.
 * ========================================================================================== */

#define SF_POSE_BOXES_MAX_ANCHORS 16384
#define SF_POSE_BOXES_MAX_STRIDES 4
#define SF_POSE_BOXES_MAX_CLASSES 255
#define SF_POSE_BOXES_MAX_FRAMES 65535
#define SF_POSE_CROP_MAX_SIZE 1024
#define SF_POSE_CROP_MAX_FRAME 16384
#define SF_POSE_SIMCC_POINTS 133
#define SF_POSE_SIMCC_MAX_BINS 65536
enum sf_pose_simcc_dtype { SF_POSE_SIMCC_F32 = 0, SF_POSE_SIMCC_F16 = 1 };

typedef struct sf_pose_boxes_args {
  const float* head;          /* DEVICE float32 [F][A][5 + C], 4-byte aligned                                          */
  float* boxes;               /* DEVICE float32 [F][P][5] = (x1, y1, x2, y2, score) in descending score, then (-1, -1, -1, -1, 0); every element is written */
  int32_t* count;             /* DEVICE int32 [F]: the boxes of each frame; every element is written                   */
  float* scratch;             /* DEVICE sf_pose_boxes_scratch_bytes(F, A) bytes, 4-byte aligned                        */
  int32_t F, A, C, P;         /* 1 <= F <= 65535, A = sum (in_h / s)(in_w / s) <= 16384, 1 <= C <= 255, 1 <= P <= SF_POSE_RENDER_MAX_PEOPLE; no two ranges overlap */
  int32_t in_h, in_w;         /* the detector's input size, a multiple of every stride                                 */
  int32_t n_strides;          /* 1 .. SF_POSE_BOXES_MAX_STRIDES                                                        */
  int32_t strides[SF_POSE_BOXES_MAX_STRIDES];
  int32_t class_index;        /* 0 .. C - 1                                                                            */
  int32_t decoded;            /* 1: o0..o3 are cx, cy, w, h already                                                    */
  float ratio;                /* the letterbox scale, fp32 min(in_h / H, in_w / W); finite, > 0                        */
  float score_threshold;      /* finite, >= 0                                                                          */
  float iou_threshold;        /* finite                                                                                */
} sf_pose_boxes_args;

int sf_pose_boxes_decode(const sf_pose_boxes_args* args, void* stream);

/* Host only: the bytes of `scratch` (F * A * 20); 0 for F or A out of range. */
size_t sf_pose_boxes_scratch_bytes(int F, int A);

typedef struct sf_pose_crop_args {
  const void* frames;         /* DEVICE uint8, F frames of H x W in `layout`                                           */
  const float* boxes;         /* DEVICE float32 [F][P][5]                                                              */
  const int32_t* count;       /* DEVICE int32 [F]                                                                      */
  void* out;                  /* DEVICE [F * P][3][out_h][out_w] in `dtype`; every element is written                  */
  int32_t F, P, H, W;         /* 1 <= F <= 65535, 1 <= P <= SF_POSE_RENDER_MAX_PEOPLE, 1 <= H, W <= SF_POSE_CROP_MAX_FRAME; no two ranges overlap */
  int32_t layout;             /* enum sf_jpeg_layout                                                                   */
  int32_t out_h, out_w;       /* 1 .. SF_POSE_CROP_MAX_SIZE                                                            */
  int32_t dtype;              /* SF_JPEG_F32 or SF_JPEG_BF16 (round-to-nearest-even of the float32 value)              */
  int32_t bgr;                /* 1: output channel c is the frame's channel 2 - c                                      */
  float padding;              /* finite, > 0                                                                           */
  float mean[3], std[3];      /* by OUTPUT channel; finite, std > 0                                                    */
} sf_pose_crop_args;

int sf_pose_crop_people(const sf_pose_crop_args* args, void* stream);

typedef struct sf_pose_simcc_args {
  const void* simcc_x;        /* DEVICE [F * P][133][Wx] in `dtype`                                                    */
  const void* simcc_y;        /* DEVICE [F * P][133][Wy] in `dtype`                                                    */
  const float* boxes;         /* DEVICE float32 [F][P][5]                                                              */
  const int32_t* count;       /* DEVICE int32 [F]                                                                      */
  float* out;                 /* DEVICE float32 [F][P][134][3]; every element is written                               */
  const uint8_t* order;       /* HOST uint8 [134], each < 134: out[i] = tmp[order[i]]                                  */
  int32_t F, P, H, W;         /* as sf_pose_crop_args: the frame the boxes are in                                      */
  int32_t Wx, Wy;             /* 1 .. SF_POSE_SIMCC_MAX_BINS                                                           */
  int32_t dtype;              /* enum sf_pose_simcc_dtype; float16 widens exactly                                      */
  int32_t out_h, out_w;       /* the crop's size, 1 .. SF_POSE_CROP_MAX_SIZE                                           */
  int32_t normalized;         /* 1: x / W, y / H; 0: source-frame pixels                                               */
  float padding;              /* as the crop's                                                                         */
  float split_ratio;          /* bins per crop pixel; finite, > 0                                                      */
  float neck_threshold;       /* finite                                                                                */
} sf_pose_simcc_args;

int sf_pose_simcc_decode(const sf_pose_simcc_args* args, void* stream);

/* ==========================================================================================
 * Pose front end (DWPose frames -> pose tokens): `dwpose_embedding` and `randomref_embedding_pose` of the many-step
 * sampler (pipeline/causal_diffusion_inference.py:87-122) with their input transform (:337-343).  Runs once per clip.
 * Activations are channels-last bf16 volumes [T][H][W][C] with C = 8 (the three input channels, stored padded with
 * zeros) or 16.  Every volume must stay under 4 GiB (32-bit byte offsets); larger ones are refused.
 * ========================================================================================== */

enum sf_pose_dtype { SF_POSE_U8 = 0, SF_POSE_F32 = 1, SF_POSE_BF16 = 2 };

/* Output size of the stacks' layers along one axis: kernel 3 with padding 1, or kernel 2 without padding
 * (nn.Conv3d / nn.Conv2d arithmetic, causal_diffusion_inference.py:90-102, :110-120). */
int sf_pose_out_size(int n, int kernel, int stride);

/* One convolution of the stacks, fp32 accumulation on the matrix cores, fp32 bias, optional SiLU, one rounding:
 *   out[(t,h,w)][n] = act(bias[n] + sum_{dt<kt,dh,dw,ci} x[t*st-pt+dt][h*ss-1+dh][w*ss-1+dw][ci] * w[n][((dt*3+dh)*3+dw)*Cin+ci])
 * with symmetric zero padding (pt = 1 for kt = 3, else 0).  Replaces nn.Conv3d 3x3x3 / nn.Conv2d 3x3 (kt = 1, T = 1) and
 * the nn.SiLU behind it (causal_diffusion_inference.py:90-101, :110-120).  Supported: (Cin, kt, stride_t, stride_s) in
 * (8|16, 3, 1, 1), (16, 3, 1, 2), (16, 3, 2, 2), (8|16, 1, 1, 1), (16, 1, 1, 2); Cout <= 16, or <= 32 for (16, 1, 1, 2). */
typedef struct sf_pose_conv_args {
  const void* x;          /* [T][H][W][Cin] bf16                                                                  */
  const void* w;          /* [16 or 32 rows][ldw] bf16: k = tap*Cin + ci, zero padded to ldw >= roundup(kt*9*Cin, 32);
                             rows past Cout zero                                                                  */
  const float* bias;      /* fp32 [16 or 32], zero past Cout                                                      */
  void* out;              /* [Tout][Hout][Wout] rows of ldo bf16 channels; channels >= Cout are not written       */
  int32_t T, H, W;        /* input volume; Tout = (T-1)/stride_t + 1 (kt = 3) or T, Hout = (H-1)/stride_s + 1     */
  int32_t Cin, Cout;
  int32_t kt, stride_t, stride_s;
  int32_t ldw, ldo;
  int32_t silu;           /* 1: SiLU behind the bias                                                              */
} sf_pose_conv_args;

int sf_pose_conv(const sf_pose_conv_args* args, void* stream);

/* The same convolution over a temporal WINDOW of a clip, for embedding a clip piece by piece.  args->x holds the
 * clip-timeline frames [x_t0, x_t0 + args->T) of the layer's input (x_t0 may be negative: the frames in front of the
 * clip are never read); the timeline's valid range is [0, t_end): frames < 0 are zero, frames >= t_end are zero when
 * the clip is `closed` and must not be needed otherwise.  Output frames [t_out0, t_out0 + n_out) are computed (any
 * start, either parity under temporal stride 2) and output frame t_out0 is written at args->out's start.  Every output
 * element is formed from the same taps in the same order as in sf_pose_conv, so a window that holds a frame's true
 * neighbours gives the whole-clip bits; the whole-volume call is the window (0, [0, T) closed, 0, Tout).  Refused: a
 * window that does not hold every in-range input frame the outputs read (t*stride_t - 1 .. t*stride_t + 1), and a
 * window or output of 4 GiB or more.  kt = 3 only: (Cin, stride_t, stride_s) in (8|16, 1, 1), (16, 1, 2), (16, 2, 2),
 * Cout <= 16. */
typedef struct sf_pose_window {
  int32_t x_t0;           /* clip-timeline index of x's first frame                                               */
  int32_t t_end;          /* the timeline's valid range is [0, t_end)                                             */
  int32_t closed;         /* 1: the clip has ended, frames >= t_end are the zero padding; 0: they must not be read */
  int32_t t_out0, n_out;  /* output frames [t_out0, t_out0 + n_out)                                               */
} sf_pose_window;

int sf_pose_conv_window(const sf_pose_conv_args* args, const sf_pose_window* window, void* stream);

/* The input transform (causal_diffusion_inference.py:337-343): pose frames holding 0..255 as uint8 / float32 / bf16
 * (enum sf_pose_dtype), planar [3][F][H][W] (hwc = 0) or one image [H][W][3] (hwc = 1, F = 1), -> bf16
 * [lead + F][H][W][8]: `lead` copies of the first frame in front (3 for the clip, :339), value / 255 (the fp32 quotient
 * rounded once), channels 3..7 zero. */
int sf_pose_prepare(const void* src, int dtype, int hwc, int F, int H, int W, int lead, void* out, void* stream);

typedef struct sf_pose_layer {
  const void* w;          /* as sf_pose_conv_args.w                                                               */
  const float* bias;      /* as sf_pose_conv_args.bias                                                            */
  int32_t cin, cout, kt, stride_t, stride_s, ldw, silu;   /* cin as stored (8 or 16)                              */
} sf_pose_layer;

#define SF_POSE_CONVS 6

typedef struct sf_pose_model {
  sf_pose_layer conv[SF_POSE_CONVS];      /* dwpose_embedding.0, .2, .4, .6, .8, .10 (:90-101)                    */
  const void* embed_w;                    /* dwpose_embedding.12 (:102) as [pose_dim][64] bf16, k = (dh*2+dw)*16+ci */
  const void* embed_b;                    /* [pose_dim] bf16                                                      */
  int32_t pose_dim;                       /* 5120                                                                 */
  sf_pose_layer ref_conv[SF_POSE_CONVS];  /* randomref_embedding_pose.0 .. .10 (:110-120), kt = 1                 */
} sf_pose_model;

/* The last layer of the dwpose stack (nn.Conv3d(16, 5120, (1,2,2), stride=(1,2,2)), causal_diffusion_inference.py:102) as
 * the patch-embed pattern: x [T][H][W][16] -> rows [T*(H/2)*(W/2)][64] (scratch; row k = (dh*2+dw)*16 + ci) ->
 * sf_gemm_bf16 with w [pose_dim][64], bias bf16 [pose_dim] -> tokens_out [T*(H/2)*(W/2)][pose_dim]. */
int sf_pose_patch_embed(const void* x, int T, int H, int W, const void* w, const void* bias, int pose_dim, void* rows,
                        void* tokens_out, void* stream);

/* Scratch of one sf_pose_embed call on F pose frames of H x W (F >= 1), or of sf_pose_embed_ref (F = 0).
 * 0 = malformed arguments or a volume of 4 GiB or more (sf_last_error says which). */
size_t sf_pose_scratch_bytes(const sf_pose_model* model, int F, int H, int W);

/* The whole dwpose stack in one host call (causal_diffusion_inference.py:337-340 with :388-391): frames [3][F][H][W]
 * -> tokens_out bf16 [F'*h*w][pose_dim], token-major -- rows [f*h*w, (f+1)*h*w) are latent frame f's `add_condition`
 * ('b c f h w -> b (f h w) c' of the reference's output).  (F', h, w) follow from sf_pose_out_size over F + 3 frames;
 * n_tokens must equal F'*h*w. */
int sf_pose_embed(const sf_pose_model* model, const void* frames, int dtype, int F, int H, int W, void* scratch,
                  size_t scratch_bytes, void* tokens_out, int64_t n_tokens, void* stream);

/* The reference-pose stack (causal_diffusion_inference.py:341-343): image [H][W][3] -> out bf16 [h][w][20],
 * channels-last (the reference's [1, 20, 1, h, w] is a permuted view). */
int sf_pose_embed_ref(const sf_pose_model* model, const void* image, int dtype, int H, int W, void* scratch,
                      size_t scratch_bytes, void* out, void* stream);

/* The dwpose stack, resumable: a clip is pushed in pieces of any length and every latent frame comes out as soon as the
 * pixel frames it depends on are in (latent frame j reads pixel frames 4j-10 .. 4j+4, so it is final once 4j+5 are
 * known), with the bits sf_pose_embed gives for the whole clip.  The library keeps no state: `state` is a caller-owned
 * device buffer holding the last two frames of each of the six layer inputs, and the position is `frames_before`.
 *
 * Level 0 is the prepared volume (three copies of frame 0, then the pixel frames), level i + 1 the output of
 * convolution i.  With P pixel frames pushed and the clip open the levels' final frames are P+3, P+2, P+1, P, P-1,
 * (P-1)/2, (P-1)/4 (all 0 for P = 0); once closed they are the full sizes sf_pose_out_size gives over P + 3 frames.
 * sf_pose_stream_plan states what a push computes: level l gains frames [first[l], first[l] + count[l]), and convolution
 * l reads them from a window of 2 + count[l] frames starting at first[l] - 2.  0 on success. */
#define SF_POSE_LEVELS (SF_POSE_CONVS + 1)
typedef struct sf_pose_push_plan {
  int32_t first[SF_POSE_LEVELS], count[SF_POSE_LEVELS];
} sf_pose_push_plan;
int sf_pose_stream_plan(int frames_before, int n, int closing, sf_pose_push_plan* plan);

/* Bytes of `state` for H x W frames (two frames per layer input); 0 = malformed arguments. */
size_t sf_pose_stream_state_bytes(const sf_pose_model* model, int H, int W);
/* Scratch of a push of up to n_max pixel frames, closing or not: independent of the clip's length.  0 = malformed
 * arguments or a window of 4 GiB or more. */
size_t sf_pose_stream_scratch_bytes(const sf_pose_model* model, int n_max, int H, int W);

/* Push n >= 0 new pixel frames [3][n][H][W] (enum sf_pose_dtype) behind the `frames_before` already pushed; `closing`
 * declares the clip ended after them (n = 0 then flushes the tail; a clip of no frames cannot be closed).  The rows of
 * the latent frames this push makes final are written token-major at tokens_out ([frames*h*w][pose_dim] bf16, at most
 * token_rows_capacity rows) and their number of frames at *latent_frames_written; a push that finalises nothing writes
 * 0 frames.  state: 256-byte aligned, untouched contents on the first push (frames_before = 0). */
int sf_pose_stream_push(const sf_pose_model* model, void* state, int frames_before, const void* frames, int dtype, int n,
                        int H, int W, int closing, void* scratch, size_t scratch_bytes, void* tokens_out,
                        int64_t token_rows_capacity, int32_t* latent_frames_written, void* stream);

/* ==========================================================================================
 * umT5 text encoder (prompt token ids -> prompt embeddings): WanTextEncoder.forward after its tokenizer
 * (utils/wan_wrapper.py:40-55) -> T5Encoder.forward (wan/modules/t5.py:299-312).  Runs once per prompt.
 * ========================================================================================== */

/* nn.Embedding lookup: out[t][:] = table[ids[t]][:] (ids int64; an id outside [0, vocab) is an error
 * reported by the caller -- the kernel clamps). */
int sf_embedding_gather(const int64_t* ids, const void* table, void* out, int n_tokens, int dim, int vocab,
                        void* stream);

/* Logits -> probabilities of T5Attention (t5.py:104-118) for all heads of one sample:
 *   p[h][i][j] = softmax_j( s[h][i][j] + emb[rel_bucket[j - i + L - 1]][h] + (key_mask[j] ? 0 : -inf) ),  j < L
 *   p[h][i][j] = 0 for L <= j < ld  (zero padding so that p can be the A operand of a K = ld GEMM)
 * s float32 [H][L][ld], p bf16 [H][L][ld], emb bf16 [num_buckets][H] (T5RelativeEmbedding.embedding.weight),
 * rel_bucket int32 [2L-1] (host-computed bucket of every relative position, t5.py:236-256), key_mask int64 [L]. */
int sf_t5_softmax_bias(const float* s, void* p, const void* emb, const int32_t* rel_bucket, const int64_t* key_mask,
                       int H, int L, int ld, void* stream);

/* out[i] = a[i] * b[i] (bf16; the gated-GELU product fc1(x) * gelu(gate(x)), t5.py:138); in place allowed. */
int sf_mul_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);

/* rows of x [B*L][dim] whose mask entry is 0 are set to zero (WanTextEncoder.forward, wan_wrapper.py:50-51). */
int sf_zero_masked_rows(void* x, const int64_t* mask, int rows, int dim, void* stream);

typedef struct sf_t5_layer {       /* T5SelfAttention, t5.py:146-178 */
  const void* norm1_w;             /* [dim] */
  const void* qk_w;                /* attn.q | attn.k stacked: [2*dim_attn][dim] */
  const void* v_w;                 /* [dim_attn][dim] */
  const void* o_w;                 /* [dim][dim_attn] */
  const void* norm2_w;
  const void* gate_w;              /* ffn.gate.0: [dim_ffn][dim] */
  const void* fc1_w;               /* [dim_ffn][dim] */
  const void* fc2_w;               /* [dim][dim_ffn] */
  const void* pos_emb;             /* pos_embedding.embedding.weight [num_buckets][num_heads] */
} sf_t5_layer;

typedef struct sf_t5_model {
  int32_t vocab, dim, dim_attn, dim_ffn, num_heads, num_layers, num_buckets;
  float eps;
  const void* token_embedding;     /* [vocab][dim] */
  const sf_t5_layer* layers_host;  /* HOST array [num_layers] */
  const void* final_norm_w;        /* [dim] */
} sf_t5_model;

size_t sf_t5_workspace_bytes(const sf_t5_model* model, int batch, int seq_len);
/* ids, mask: int64 [batch][seq_len] (mask 1 = token, a prefix mask); rel_bucket int32 [2 seq_len - 1];
 * out bf16 [batch][seq_len][dim], rows past each prompt's length zero. */
int sf_t5_encode(const sf_t5_model* model, const int64_t* ids, const int64_t* mask, const int32_t* rel_bucket,
                 int batch, int seq_len, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* ==========================================================================================
 * CLIP image encoder (frames -> clip_feature): CLIPModel.visual (wan/modules/clip.py:527-542) -> VisionTransformer.forward
 * with use_31_block=True (clip.py:279-297).  ViT: patch 14, head dimension 80, exact GELU, LayerNorm eps 1e-5.  The
 * residual stream is fp32 (clip.py:47-50: the norms run on x.float(), bf16 sub-layer outputs are added into an fp32 x);
 * every matrix product is sf_gemm_bf16 with SF_EPI_BIAS.  Runs once per conditioning image.
 * ========================================================================================== */

enum sf_clip_dtype { SF_CLIP_F32 = 0, SF_CLIP_BF16 = 1 };

/* CLIPModel.visual's preprocessing (clip.py:529-537): frames [n][3][H][W] (dtype: sf_clip_dtype) in [-1, 1] ->
 * F.interpolate(size = image_size, mode = 'bicubic', align_corners = False) (A = -0.75, taps clamped to the edge, no
 * antialiasing, overshoot kept) -> (v/2 + 1/2 - mean_c) / std_c, written as bf16 patch rows for the patch-embedding GEMM:
 * rows [n * (image_size/patch)^2][kp], row = (frame, patch row-major), column k = (c*patch + i)*patch + j for pixel (i, j)
 * of the patch; columns 3*patch^2 <= k < kp are zero.  kp >= 3*patch^2, image_size % patch == 0. */
int sf_clip_preprocess(const void* frames, int dtype, int n, int H, int W, int image_size, int patch, int kp, void* rows,
                       void* stream);

/* Start of the fp32 residual stream, x32 [n*L][dim] with L = P + 1:
 *   x32[b][0] = cls + pos[0];  x32[b][1 + p] = float(patch_out[b*P + p]) + pos[1 + p];  x32 = LN(x32; pre_w, pre_b)
 * and its first normalised copy xn bf16 [n*L][dim] = LN(x32; ln_w, ln_b) (norm1 of block 0).  patch_out bf16 [n*P][dim];
 * cls [dim], pos [L][dim] and the norm vectors are fp32; statistics in fp32.  With ln_w == NULL only the stream is
 * written (ln_b, xn may be NULL).  dim % 4 == 0, dim <= 8192. */
int sf_clip_embed_norm(const void* patch_out, const float* cls, const float* pos, const float* pre_w, const float* pre_b,
                       const float* ln_w, const float* ln_b, float* x32, void* xn, int n, int P, int dim, float eps, void* stream);

/* Fused residual add and LayerNorm on the fp32 stream: x32[r][:] += float(y[r][:]) (y bf16 [rows][dim]); with ln_w the
 * normalised copy xn = bf16(LN(x32[r]) * ln_w + ln_b) is written too (fp32 statistics, one pass over the row in memory);
 * with ln_w == NULL only the add happens and xn is not touched (ln_b, xn may be NULL).  dim % 4 == 0, dim <= 8192. */
int sf_clip_add_layernorm(float* x32, const void* y, const float* ln_w, const float* ln_b, void* xn, int rows, int dim, float eps,
                          void* stream);

/* Non-causal softmax attention at head dimension 80, straight off the packed projection: qkv bf16 [n][L][3][H][80] (the
 * memory layout of to_qkv(x).view(b, s, 3, n, d), clip.py:81) -> out bf16 [n][L][H*80]; scale 1/sqrt(80), scores and softmax
 * in fp32, probabilities rounded to bf16 in front of P.V.  K and V of one (image, head) stay in LDS: 1 <= L <= 480. */
int sf_clip_attention(const void* qkv, void* out, int n, int L, int H, void* stream);

/* nn.GELU() (erf form), evaluated in fp32: out[i] = bf16(x[i] * Phi(x[i])), bf16 [count]; in place allowed. count % 8 == 0. */
int sf_clip_gelu(const void* x, void* out, int64_t count, void* stream);

typedef struct sf_clip_layer {     /* AttentionBlock, clip.py:112-153 */
  const float* norm1_w;            /* [dim] fp32 */
  const float* norm1_b;
  const void* qkv_w;               /* attn.to_qkv.weight bf16 [3*dim][dim] */
  const void* qkv_b;               /* bf16 [3*dim] */
  const void* proj_w;              /* attn.proj.weight bf16 [dim][dim] */
  const void* proj_b;
  const float* norm2_w;
  const float* norm2_b;
  const void* fc1_w;               /* mlp.0.weight bf16 [mlp_dim][dim] */
  const void* fc1_b;
  const void* fc2_w;               /* mlp.2.weight bf16 [dim][mlp_dim] */
  const void* fc2_b;
} sf_clip_layer;

typedef struct sf_clip_model {
  int32_t image_size, patch, dim, heads, mlp_dim, layers_built;
  float eps;
  const void* patch_w;             /* patch_embedding.weight repacked bf16 [dim][kp], kp = 3*patch^2 rounded up to 64 */
  const float* cls;                /* cls_embedding fp32 [dim] */
  const float* pos;                /* pos_embedding fp32 [(image_size/patch)^2 + 1][dim] */
  const float* pre_norm_w;         /* fp32 [dim] */
  const float* pre_norm_b;
  const sf_clip_layer* layers_host; /* HOST array [layers_built]: every block but the last (use_31_block) */
} sf_clip_model;

size_t sf_clip_workspace_bytes(const sf_clip_model* model, int n);
/* frames [n][3][H][W] (dtype: sf_clip_dtype) -> out fp32 [n][(image_size/patch)^2 + 1][dim], the un-normed stream after
 * the last built block.  `out` is the residual stream itself: it is written throughout the call. */
int sf_clip_encode(const sf_clip_model* model, const void* frames, int dtype, int n, int H, int W, float* out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measured ceilings of the box ("Peaks to divide by": "re-measure on the box (a peak-MFMA micro-kernel
 * and a streaming-copy kernel) and use the measured ceilings in the fraction").  Measurement entry points for
 * bench.py (roofline.measured_peak, hbm_measured_peak); no product kernel depends on them and the reference has no
 * counterpart.
 *   sf_probe_mfma: `workgroups` x 4 waves each issue iters x 32 v_mfma_f32_32x32x16_bf16 (shape 0) or iters x 64
 *                  v_mfma_f32_16x16x32_bf16 (shape 1) from registers, 4 independent accumulators; `operands` = 8 KiB
 *                  of (random) bf16, `sink` = workgroups * 256 floats; *flops_out (HOST, optional) = flops of the launch.
 *   sf_probe_copy: streaming copy of `bytes` (multiple of 16) from src to dst, 16 bytes per lane. */
int sf_probe_mfma(int shape, int iters, int workgroups, const void* operands, float* sink, double* flops_out_host,
                  void* stream);
int sf_probe_copy(const void* src, void* dst, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SF_HIP_H */
