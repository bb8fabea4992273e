// One whole denoiser pass of the causal Wan DiT as a single host call that enqueues every kernel
// on the caller's stream: CausalWanModel._forward_inference (wan/modules/causal_model.py:725-893)
// + the wrapper's flow -> x0 conversion (utils/wan_wrapper.py:288-300, :340-344).
//
// Host-side only (no kernels here): carves the caller's workspace and sequences the C-ABI
// launchers.  No allocation, no synchronisation, no device read-back: cache indices arrive as
// host integers (the pipeline always knows them), so the reference's >= 60 `.item()` syncs per
// forward (causal_model.py:207-226) disappear.
#include <algorithm>
#include "sf_host.h"

int sf_internal_write_kv_indices(void* buf, int layers, int64_t global_end, int64_t local_end, void* stream);   // elementwise.hip

namespace {

struct Work {
  void *x, *xn, *qkv, *q, *att, *hbuf, *cols, *headout, *sin, *etmp, *e, *e0, *ctx1, *ctx;
  void* xq;        // fp8 only: the e4m3 copy of the current Linear input (one at a time: the GEMMs run in stream order)
  float* xs;       // fp8 only: its scales (one per pass) + the quantiser's scratch
  size_t total;
};

constexpr int FP8_MAX_SEGMENTS = 8;   // scale slots: one per pass of a call (1 or 2)

Work carve(const sf_model* m, void* ws, int B, int F, int lat_h, int lat_w, int groups) {
  const size_t M = (size_t)B * F * (lat_h / 2) * (lat_w / 2);
  const size_t C = m->dim, BG = (size_t)B * groups, T = (size_t)B * m->text_len;
  Carve c(ws);
  Work w;
  w.x = c.take(M * C * 2);
  w.xn = c.take(M * C * 2);
  w.qkv = c.take(M * 3 * C * 2);
  w.q = c.take(M * C * 2);
  w.att = c.take(M * C * 2);
  w.hbuf = c.take(M * (size_t)m->ffn_dim * 2);
  w.cols = c.take(M * (size_t)m->in_dim * 4 * 2);
  w.headout = c.take(M * (size_t)m->out_dim * 4 * 2);
  w.sin = c.take(BG * m->freq_dim * 2);
  w.etmp = c.take(BG * C * 2);
  w.e = c.take(BG * C * 2);
  w.e0 = c.take(BG * 6 * C * 2);
  w.ctx1 = c.take(T * C * 2);
  w.ctx = c.take(T * C * 2);
  w.xq = nullptr;
  w.xs = nullptr;
  if (m->fp8) {
    const size_t pose = m->pose_dim > 0 ? (size_t)m->pose_dim : C;
    const size_t widest_tok = std::max({(size_t)m->ffn_dim, C, pose}), widest_txt = std::max((size_t)m->text_dim, C);
    w.xq = c.take(std::max(M * widest_tok, T * widest_txt));
    w.xs = (float*)c.take(FP8_MAX_SEGMENTS * (1 + SF_FP8_AMAX_PARTS) * sizeof(float));
  }
  w.total = c.off;
  return w;
}

inline const char* bptr(const void* p, size_t elems) { return (const char*)p + elems * 2; }

// The i2v model type's image context buffers, carved BEHIND the t2v workspace so that nothing in front of them moves.
struct ImgWork {
  void *t0, *t1, *ctx;   // [B clip_len, clip_dim] x 2 (LayerNorm / Linear ping-pong), [B clip_len, C] x 2 in ctx (fc2 out | normed)
  size_t total;
};
ImgWork carve_img(const sf_model* m, const sf_i2v_model* im, void* ws, size_t base, int B) {
  const size_t R = (size_t)B * im->clip_len;
  Carve c(ws);
  c.off = base;
  ImgWork w;
  w.t0 = c.take(R * im->clip_dim * 2);
  w.t1 = c.take(R * im->clip_dim * 2);
  w.ctx = c.take(2 * R * (size_t)m->dim * 2);
  w.total = c.off;
  return w;
}

}  // namespace

extern "C" size_t sf_dit_workspace_bytes(const sf_model* model, const sf_i2v_model* i2v_model, int batch, int frames, int lat_h, int lat_w,
                                         int groups) {
  if (!model || batch <= 0 || frames <= 0 || lat_h <= 0 || lat_w <= 0 || groups <= 0) return 0;
  const size_t base = carve(model, nullptr, batch, frames, lat_h, lat_w, groups).total;
  if (!i2v_model) return base;
  if (!base || i2v_model->clip_len <= 0 || i2v_model->clip_dim <= 0) return 0;
  return carve_img(model, i2v_model, nullptr, base, batch).total;
}

// ------------------------------------------------------------------------------------------
// The pass sequencer.  `np` passes (1 or 2) over the SAME model, caches and latent geometry run
// as ONE batch of np * B samples through everything that is row-wise -- patch embedding, time MLPs, norms, all ten GEMMs
// of a layer, the head -- and one after the other through what touches the KV cache (eviction, K / V write, attention:
// pass p + 1's write and eviction must not be visible to pass p's attention, exactly as when the passes run as separate
// calls).  Row-wise kernels compute every output row from that row alone and every GEMM tiling keeps the k order per
// output element, so the results are bit-identical to separate calls; what changes is M (two passes of 4680 tokens give
// the GEMMs 9360 rows: 1040-1440 instead of 810-1160 TFLOP/s) and the launch count.
// cache_only passes must come first; past the LAST layer's K / V write only the remaining passes' rows continue.
// `im` / `ia` (NULL for a t2v generator: nothing below changes) add the i2v model type: the 36-channel patch gather, the
// image context with init_cross, and the image attention accumulated behind every layer's text attention.
extern "C" int sf_dit_forward(const sf_model* m, const sf_forward_call* call, void* stream) {
  SF_CHECK(m && call, "sf_dit_forward: null argument");
  const sf_forward_args* const* ps = call->passes;
  const int np = call->n_passes;
  SF_CHECK(np == 1 || np == 2, "sf_dit_forward: one or two passes per call (n_passes=%d)", np);
  const sf_forward_args* a = ps[0];
  SF_CHECK(a && ps[np - 1], "sf_dit_forward: null argument");
  SF_CHECK(ps[np - 1]->workspace == a->workspace && ps[np - 1]->workspace_bytes == a->workspace_bytes,
           "sf_dit_forward: both passes name the same workspace (sized for 2 x batch)");
  int32_t* const cross_keys = call->cross_keys;
  float* const cross_log2w = call->cross_log2w;
  SF_CHECK((cross_keys == nullptr) == (cross_log2w == nullptr), "sf_dit_forward: cross_keys and cross_log2w come together");
  const sf_i2v_model* const im = call->i2v_model;
  const sf_i2v_args* const ia = call->i2v_args;
  SF_CHECK((im == nullptr) == (ia == nullptr), "sf_dit_forward: null argument (i2v_model and i2v_args come together)");
  if (im) {
    SF_CHECK(np == 1, "sf_dit_forward: the two-pass call is not built for the i2v model type");
    SF_CHECK(!m->fp8, "sf_dit_forward: fp8 Linears are not built for the i2v model type");
    SF_CHECK(im->layers_host && im->clip_len > 0 && im->clip_dim > 0 && im->clip_dim % 64 == 0,
             "sf_dit_forward: bad image context shape (clip_len=%d, clip_dim=%d: a positive multiple of 64)", im->clip_len, im->clip_dim);
    SF_CHECK(ia->y, "sf_dit_forward: y is missing (an i2v generator needs clip_feature and y)");
    SF_CHECK(m->in_dim >= m->out_dim + ia->y_channels && ia->y_channels > 0 && (m->in_dim * 4) % 64 == 0,
             "sf_dit_forward: %d latent + %d conditioning channels do not fit the padded in_dim %d", m->out_dim, ia->y_channels, m->in_dim);
    SF_CHECK(ia->kimg_cache_host && ia->vimg_cache_host, "sf_dit_forward: null image cache table");
    SF_CHECK(!a->init_cross || ia->clip_feature, "sf_dit_forward: init_cross needs clip_feature");
  }
  SF_CHECK(m->layers_host && m->num_layers > 0, "sf_dit_forward: model has no layers");
  SF_CHECK(m->dim == m->num_heads * 128, "sf_dit_forward: head_dim must be 128 (dim=%d heads=%d)", m->dim, m->num_heads);
  SF_CHECK(a->batch > 0 && a->frames > 0 && a->groups > 0, "sf_dit_forward: empty input");
  SF_CHECK(a->lat_h % 2 == 0 && a->lat_w % 2 == 0, "sf_dit_forward: latent size must be even");
  const int B = a->batch, F = a->frames, h = a->lat_h / 2, w = a->lat_w / 2;
  const int L = F * h * w, M = B * L, C = m->dim, G = a->groups, BG = B * G;
  const int Mt = np * M, BGt = np * BG;                    // rows / modulation groups of the whole batch of passes
  SF_CHECK(F % G == 0, "sf_dit_forward: frames=%d not divisible by timestep groups=%d", F, G);
  const int rpg = L / G;
  SF_CHECK(BGt <= 32, "sf_dit_forward: passes*batch*groups=%d exceeds the small-linear limit of 32", BGt);
  int first_full = np;                                      // first pass that runs to the end
  for (int p = 0; p < np; ++p) {
    const sf_forward_args* q = ps[p];
    SF_CHECK(q, "sf_dit_forward: null pass");
    SF_CHECK(q->batch == B && q->frames == F && q->lat_h == a->lat_h && q->lat_w == a->lat_w && q->groups == G,
             "sf_dit_forward: the passes of one call must share batch, frames, latent size and timestep groups");
    SF_CHECK(q->k_cache_host == a->k_cache_host && q->v_cache_host == a->v_cache_host && q->ck_cache_host == a->ck_cache_host &&
             q->cv_cache_host == a->cv_cache_host && q->cache_tokens == a->cache_tokens, "sf_dit_forward: the passes of one call must share their caches");
    SF_CHECK(q->noisy && q->timestep, "sf_dit_forward: null tensor");
    SF_CHECK(q->cache_only || (q->flow_out && q->x0_out), "sf_dit_forward: null output tensor");
    SF_CHECK(q->attn_start >= 0 && q->attn_end > q->attn_start && q->attn_end <= q->cache_tokens, "sf_dit_forward: bad attention window [%d, %d) of %lld",
             q->attn_start, q->attn_end, (long long)q->cache_tokens);
    SF_CHECK(q->write_start >= 0 && (int64_t)q->write_start + L <= q->cache_tokens,
             "sf_dit_forward: KV cache overflow: write_start=%d + %d new tokens > capacity %lld", q->write_start, L, (long long)q->cache_tokens);
    SF_CHECK(q->write_start + L == q->attn_end, "sf_dit_forward: the new tokens must end the attention window");
    if (q->evict > 0) SF_CHECK(q->evict_scratch && q->keep >= 0, "sf_dit_forward: eviction needs evict_scratch");
    SF_CHECK(np == 1 || !q->init_cross, "sf_dit_forward: the cross-attention cache must be initialised by an earlier single pass");
    if (!q->cache_only && first_full == np) first_full = p;
    SF_CHECK(!(q->cache_only && first_full != np), "sf_dit_forward: cache_only passes must come first");
  }
  SF_CHECK(a->k_cache_host && a->v_cache_host && a->ck_cache_host && a->cv_cache_host, "sf_dit_forward: null cache table");
  const Work ws = carve(m, a->workspace, np * B, F, a->lat_h, a->lat_w, G);
  const size_t ws_need = im ? carve_img(m, im, nullptr, ws.total, B).total : ws.total;
  SF_CHECK(a->workspace && a->workspace_bytes >= ws_need, "sf_dit_forward: workspace too small (%zu < %zu)", a->workspace_bytes, ws_need);
  SF_CHECK(!a->init_cross || a->prompt_embeds, "sf_dit_forward: init_cross needs prompt_embeds");

  const bool f8 = m->fp8 != 0;
  static const sf_layer_fp8 no_fp8 = {};
  SF_CHECK(!f8 || m->layers_fp8_host, "sf_dit_forward: fp8 model without per-layer fp8 weights");
  // One Linear: the bf16 GEMM on w exactly as without fp8, or (fp8) the e4m3 GEMM on the weight named by fp8w() with its
  // column scales.  `run` reads the input already quantised in the workspace; `lin` quantises it first, with one scale
  // per rows_per_segment rows (= one pass).
  auto run = [&](const Gemm& g) -> int { return f8 ? g.fp8(ws.xq, ws.xs, stream) : g.bf16(stream); };
  auto lin = [&](const Gemm& g) -> int {
    if (f8) SF_TRY(sf_quantize_fp8(g.g.a, g.g.lda, g.g.M, g.g.K, g.rows_per_segment, ws.xq, ws.xs, stream));
    return run(g);
  };
  // the time MLPs: rows of one pass = one segment
  auto small = [&](const void* x, const void* w16, const void* w8, const float* s8, const void* bias, void* out, int N, int K, int act_in,
                   int act_out) -> int {
    if (!f8) return sf_small_linear(x, w16, bias, out, BGt, N, K, act_in, act_out, stream);
    return sf_small_linear_fp8(x, w8, s8, bias, out, BGt, N, K, BG, act_in, act_out, stream);
  };

  const int Kp = m->in_dim * 4, Nh = m->out_dim * 4;
  const long cache_b = (long)a->cache_tokens * C;
  const long ctx_b = (long)m->text_len * C;
  const sf_forward_args* last = ps[np - 1];
  auto finish_indices = [&]() -> int {
    if (last->kv_index_out) return sf_internal_write_kv_indices(last->kv_index_out, m->num_layers, last->global_end, last->attn_end, stream);
    return 0;
  };

  // ---- patch embedding (rows of pass p at [p M, (p + 1) M))
  if (im)   // x | y | zeros: the K = in_dim * 4 operand (in_dim is the padded 48 of an i2v sf_model)
    SF_TRY(sf_patchify_i2v(a->noisy, ia->y, ws.cols, B, F, m->out_dim, ia->y_channels, m->in_dim, a->lat_h, a->lat_w, ia->y_bstride,
                           ia->y_cstride, ia->y_fstride, stream));
  else
    for (int p = 0; p < np; ++p)
      SF_TRY(sf_patchify(ps[p]->noisy, (void*)bptr(ws.cols, (size_t)p * M * Kp), B, F, m->in_dim, a->lat_h, a->lat_w, stream));
  SF_TRY(Gemm(ws.cols, Kp, m->patch_w, Kp, ws.x, C, Mt, C, Kp).bias(m->patch_b).bf16(stream));

  // ---- pose conditioning of the fork: x += pose_proj(add_condition)  (causal_model.py:786-819), per pass
  for (int p = 0; p < np; ++p) {
    if (!ps[p]->add_condition) continue;
    void* xp = (void*)bptr(ws.x, (size_t)p * M * C);
    if (m->pose_w || (f8 && m->pose_q)) {
      SF_CHECK(m->pose_dim > 0, "sf_dit_forward: pose_proj weights without pose_dim");
      SF_TRY(lin(Gemm(ps[p]->add_condition, m->pose_dim, m->pose_w, m->pose_dim, xp, C, M, C, m->pose_dim).bias(m->pose_b)
                     .epi(SF_EPI_BIAS_RESID).resid(xp, C).fp8w(m->pose_q, m->pose_s, M)));
    } else {
      // dim == 5120: `pose_proj = nn.Identity()` (causal_model.py:500-503): x += add_condition, [M, C] bf16, fp32 add, one rounding
      SF_CHECK(m->pose_dim == C, "sf_dit_forward: add_condition without pose_proj weights needs pose_dim == dim (%d != %d)", m->pose_dim, C);
      const void* terms[2] = {xp, ps[p]->add_condition};
      const float ones[2] = {1.0f, 1.0f};
      SF_TRY(sf_lincomb_bf16(xp, terms, ones, 2, (int64_t)M * C, stream));
    }
  }

  // ---- time embeddings: e [BGt, C], e0 [BGt, 6C]  (group rows pass-major, like the token rows)
  for (int p = 0; p < np; ++p)
    SF_TRY(sf_sinusoid_embedding(ps[p]->timestep, ps[p]->t_is_int64, (void*)bptr(ws.sin, (size_t)p * BG * m->freq_dim), BG, m->freq_dim, stream));
  SF_TRY(small(ws.sin, m->time0_w, m->time0_q, m->time0_s, m->time0_b, ws.etmp, C, m->freq_dim, 0, 1));
  SF_TRY(small(ws.etmp, m->time2_w, m->time2_q, m->time2_s, m->time2_b, ws.e, C, C, 0, 0));
  SF_TRY(small(ws.e, m->tproj_w, m->tproj_q, m->tproj_s, m->tproj_b, ws.e0, 6 * C, C, 1, 0));

  // ---- text embedding + cross-attention K/V: once per prompt (the reference recomputes the text
  // MLP on every forward although only the first call consumes it, causal_model.py:837-842)
  if (a->init_cross) {
    const int T = B * m->text_len;
    SF_TRY(lin(Gemm(a->prompt_embeds, m->text_dim, m->text0_w, m->text_dim, ws.ctx1, C, T, C, m->text_dim).bias(m->text0_b).epi(SF_EPI_BIAS_GELU)
                   .fp8w(m->text0_q, m->text0_s, T)));
    SF_TRY(lin(Gemm(ws.ctx1, C, m->text2_w, C, ws.ctx, C, T, C, C).bias(m->text2_b).fp8w(m->text2_q, m->text2_s, T)));
    // fp8: the text context is quantised once (one segment: the call's B samples) and read by every layer's k and v
    if (f8) SF_TRY(sf_quantize_fp8(ws.ctx, C, T, C, T, ws.xq, ws.xs, stream));
    for (int l = 0; l < m->num_layers; ++l) {
      const sf_layer_weights& lw = m->layers_host[l];
      const sf_layer_fp8& lq = f8 ? m->layers_fp8_host[l] : no_fp8;
      SF_TRY(run(Gemm(ws.ctx, C, lw.ckv_w, C, a->ck_cache_host[l], C, T, C, C).bias(lw.ckv_b).fp8w(lq.ckv_q, lq.ckv_s, T)));
      SF_TRY(sf_rmsnorm(a->ck_cache_host[l], C, lw.cnorm_k_w, a->ck_cache_host[l], C, T, C, m->eps, stream));
      SF_TRY(run(Gemm(ws.ctx, C, bptr(lw.ckv_w, (size_t)C * C), C, a->cv_cache_host[l], C, T, C, C).bias(bptr(lw.ckv_b, C))
                     .fp8w(f8 ? (const char*)lq.ckv_q + (size_t)C * C : nullptr, f8 ? lq.ckv_s + C : nullptr, T)));
    }
    // how many trailing rows of each layer's and sample's K / V repeat the last one (the prompt's padding): folded into one key
    if (cross_keys) SF_TRY(sf_cross_fold_scan(a->ck_cache_host, a->cv_cache_host, m->num_layers, B, m->text_len, C, cross_keys, cross_log2w, stream));
    // the image context, img_emb = MLPProj (model.py:469-481): LayerNorm, Linear, erf-GELU, Linear, LayerNorm -> clip_len
    // tokens per sample, then every layer's k_img (RMS-normed) / v_img beside its text K / V
    if (im) {
      const ImgWork iw = carve_img(m, im, a->workspace, ws.total, B);
      const int R = B * im->clip_len, D = im->clip_dim;
      void* ctx_raw = iw.ctx;
      void* ctx_img = (void*)bptr(iw.ctx, (size_t)R * C);
      SF_TRY(sf_layernorm_rows(ia->clip_feature, im->img_ln0_w, im->img_ln0_b, iw.t0, R, D, im->img_eps, stream));
      SF_TRY(Gemm(iw.t0, D, im->img_fc1_w, D, iw.t1, D, R, D, D).bias(im->img_fc1_b).bf16(stream));
      SF_TRY(sf_clip_gelu(iw.t1, iw.t1, (int64_t)R * D, stream));
      SF_TRY(Gemm(iw.t1, D, im->img_fc2_w, D, ctx_raw, C, R, C, D).bias(im->img_fc2_b).bf16(stream));
      SF_TRY(sf_layernorm_affine(ctx_raw, im->img_ln1_w, im->img_ln1_b, ctx_img, R, C, im->img_eps, stream));
      for (int l = 0; l < m->num_layers; ++l) {
        const sf_i2v_layer& il = im->layers_host[l];
        SF_TRY(Gemm(ctx_img, C, il.kvimg_w, C, ia->kimg_cache_host[l], C, R, C, C).bias(il.kvimg_b).bf16(stream));
        SF_TRY(sf_rmsnorm(ia->kimg_cache_host[l], C, il.norm_k_img_w, ia->kimg_cache_host[l], C, R, C, m->eps, stream));
        SF_TRY(Gemm(ctx_img, C, bptr(il.kvimg_w, (size_t)C * C), C, ia->vimg_cache_host[l], C, R, C, C).bias(bptr(il.kvimg_b, C)).bf16(stream));
      }
    }
  }

  // ---- transformer blocks
  for (int l = 0; l < m->num_layers; ++l) {
    const sf_layer_weights& lw = m->layers_host[l];
    const sf_layer_fp8& lq = f8 ? m->layers_fp8_host[l] : no_fp8;
    const void* mod = lw.modulation;
    const bool last_layer = l == m->num_layers - 1;
    // self attention: LN + q|k|v projection for every pass at once ...
    SF_TRY(sf_layernorm_modulate(ws.x, ws.xn, Mt, C, m->eps, bptr(mod, 0), bptr(mod, C), bptr(ws.e0, 0), bptr(ws.e0, C), 6L * C, rpg, stream));
    SF_TRY(lin(Gemm(ws.xn, C, lw.qkv_w, C, ws.qkv, 3 * C, Mt, 3 * C, C).bias(lw.qkv_b).fp8w(lq.qkv_q, lq.qkv_s, M)));
    // ... then pass by pass through the cache: eviction, K / V write, attention over the pass's own window
    for (int p = 0; p < np; ++p) {
      const sf_forward_args* q = ps[p];
      const size_t roff = (size_t)p * M;
      if (q->evict > 0) {
        SF_TRY(sf_kv_evict(q->k_cache_host[l], B, q->cache_tokens, C, q->sink_tokens, q->evict, q->keep, q->evict_scratch, q->evict_scratch_bytes, stream));
        SF_TRY(sf_kv_evict(q->v_cache_host[l], B, q->cache_tokens, C, q->sink_tokens, q->evict, q->keep, q->evict_scratch, q->evict_scratch_bytes, stream));
      }
      SF_TRY(sf_qkv_norm_rope_cache(bptr(ws.qkv, roff * 3 * C), lw.norm_q_w, lw.norm_k_w, (void*)bptr(ws.q, roff * C), q->k_cache_host[l], q->v_cache_host[l],
                                    m->rope_cos, m->rope_sin, B, F, h, w, C, m->num_heads, q->cache_tokens, q->write_start, q->start_frame, m->eps, stream));
      if (q->cache_only && last_layer) continue;            // nothing downstream of this K/V write is read
      SF_TRY(Attention(bptr(ws.q, roff * C), C, (long)L * C, bptr(q->k_cache_host[l], (size_t)q->attn_start * C), bptr(q->v_cache_host[l], (size_t)q->attn_start * C),
                       C, cache_b, (void*)bptr(ws.att, roff * C), C, (long)L * C, B, m->num_heads, L, q->attn_end - q->attn_start).run(stream));
    }
    // rows that go on: all of them, except behind the last layer's K / V write, where the cache_only passes are done
    const int p0 = last_layer ? first_full : 0;
    if (p0 == np) return finish_indices();
    const size_t r0 = (size_t)p0 * M;
    const int Mr = (np - p0) * M;
    void* x = (void*)bptr(ws.x, r0 * C);
    void* xn = (void*)bptr(ws.xn, r0 * C);
    void* qb = (void*)bptr(ws.q, r0 * C);
    void* att = (void*)bptr(ws.att, r0 * C);
    void* hb = (void*)bptr(ws.hbuf, r0 * m->ffn_dim);
    const void* e0r = bptr(ws.e0, (size_t)p0 * BG * 6 * C);
    SF_TRY(lin(Gemm(att, C, lw.o_w, C, x, C, Mr, C, C).bias(lw.o_b).epi(SF_EPI_BIAS_GATE_RESID).resid(x, C)
                   .gate(bptr(mod, 2 * (size_t)C), bptr(e0r, 2 * (size_t)C), 6L * C, rpg).fp8w(lq.o_q, lq.o_s, M)));
    // cross attention
    SF_TRY(sf_layernorm_affine(x, lw.norm3_w, lw.norm3_b, xn, Mr, C, m->eps, stream));
    SF_TRY(lin(Gemm(xn, C, lw.cq_w, C, qb, C, Mr, C, C).bias(lw.cq_b).fp8w(lq.cq_q, lq.cq_s, M)));
    SF_TRY(sf_rmsnorm(qb, C, lw.cnorm_q_w, qb, C, Mr, C, m->eps, stream));
    for (int p = p0; p < np; ++p)                            // every pass reads the same text K / V: one launch per pass
      SF_TRY(Attention(bptr(ws.q, (size_t)p * M * C), C, (long)L * C, a->ck_cache_host[l], a->cv_cache_host[l], C, ctx_b, (void*)bptr(ws.att, (size_t)p * M * C), C,
                       (long)L * C, B, m->num_heads, L, m->text_len)
                 .fold(cross_keys ? cross_keys + (size_t)l * B : nullptr, cross_keys ? cross_log2w + (size_t)l * B : nullptr).run(stream));
    if (im)   // + attn(q, k_img, v_img): added into the text attention's buffer in fp32, rounded once (model.py:254-263)
      SF_TRY(Attention(ws.q, C, (long)L * C, ia->kimg_cache_host[l], ia->vimg_cache_host[l], C, (long)im->clip_len * C, ws.att, C, (long)L * C, B, m->num_heads, L,
                       im->clip_len).accum().run(stream));
    SF_TRY(lin(Gemm(att, C, lw.co_w, C, x, C, Mr, C, C).bias(lw.co_b).epi(SF_EPI_BIAS_RESID).resid(x, C).fp8w(lq.co_q, lq.co_s, M)));
    // feed forward
    SF_TRY(sf_layernorm_modulate(x, xn, Mr, C, m->eps, bptr(mod, 3 * (size_t)C), bptr(mod, 4 * (size_t)C), bptr(e0r, 3 * (size_t)C),
                                 bptr(e0r, 4 * (size_t)C), 6L * C, rpg, stream));
    SF_TRY(lin(Gemm(xn, C, lw.ffn0_w, C, hb, m->ffn_dim, Mr, m->ffn_dim, C).bias(lw.ffn0_b).epi(SF_EPI_BIAS_GELU).fp8w(lq.ffn0_q, lq.ffn0_s, M)));
    SF_TRY(lin(Gemm(hb, m->ffn_dim, lw.ffn2_w, m->ffn_dim, x, C, Mr, C, m->ffn_dim).bias(lw.ffn2_b).epi(SF_EPI_BIAS_GATE_RESID).resid(x, C)
                   .gate(bptr(mod, 5 * (size_t)C), bptr(e0r, 5 * (size_t)C), 6L * C, rpg).fp8w(lq.ffn2_q, lq.ffn2_s, M)));
  }

  // ---- head (modulated by e, not e0: causal_model.py:890, :364-366), unpatchify, flow -> x0: the passes that run to the end
  {
    const size_t r0 = (size_t)first_full * M;
    const int Mr = (np - first_full) * M;
    const void* er = bptr(ws.e, (size_t)first_full * BG * C);
    SF_TRY(sf_layernorm_modulate(bptr(ws.x, r0 * C), (void*)bptr(ws.xn, r0 * C), Mr, C, m->eps, bptr(m->head_mod, 0), bptr(m->head_mod, C), er, er, (long)C, rpg, stream));
    SF_TRY(lin(Gemm(bptr(ws.xn, r0 * C), C, m->head_w, C, (void*)bptr(ws.headout, r0 * Nh), Nh, Mr, Nh, C).bias(m->head_b)
                   .fp8w(m->head_q, m->head_s, M)));
    for (int p = first_full; p < np; ++p)
      SF_TRY(sf_unpatchify_x0(bptr(ws.headout, (size_t)p * M * Nh), ps[p]->noisy, ps[p]->timestep, ps[p]->t_is_int64, m->sched_sigmas, m->sched_timesteps, m->n_table,
                              ps[p]->flow_out, ps[p]->x0_out, B, F, G, m->out_dim, a->lat_h, a->lat_w, stream));
  }
  return finish_indices();
}
