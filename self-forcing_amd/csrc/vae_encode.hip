// The Wan VAE's chunk loop of `encode` -- WanVAE_.encode (wan/modules/vae.py:517-543) -> Encoder3d.forward with feat_cache
// (vae.py:265-367) -> conv1 and the latent normalisation -- as a host call that enqueues every kernel on the caller's stream,
// for ONE OR SEVERAL consecutive chunks of 4 pixel frames at a time (chunk 0 is the first pixel frame alone).  The mirror
// image of vae_decode.hip, with the same volumes and the same sliding history windows (vae_common.h): every causal
// convolution owns one input volume in the per-stream state, its producer writes the new frames behind two history frames,
// and a group of chunks is bit-identical to one chunk per call.
//
// Host-side only (no kernels here).  Resample 'downsample3d' (vae.py:143-160) keeps a ONE-frame cache: the frame before
// its (3,1,1) stride-2 time convolution.  Here the spatial stride-2 convolution writes its output into the time
// convolution's input volume and the time convolution starts reading at the second history frame (t_in_offset = window + 1),
// so output frame t of a chunk reads [cache | x][2t .. 2t + 2].  The first chunk after a reset skips the time convolution
// and its single frame becomes the cache (vae.py:150-152): it is simply the new frame of slot 0, which the next window
// keeps as its last history frame -- unlike the decoder's upsample3d, whose first chunk never enters the volume.
#include "vae_common.h"

namespace {

using namespace sfvae;

struct EPlan {
  int n_stages, rps, K;
  int H[SF_VAE_MAX_STAGES], W[SF_VAE_MAX_STAGES], Tmax[SF_VAE_MAX_STAGES];   // stage i: pixel size >> i, frames per chunk
  // state
  char* c1_in;
  BlockBufs blk[SF_VAE_MAX_STAGES * 8];
  char* tc[SF_VAE_MAX_STAGES];     // downsample3d: the stride-2 time convolution's input volume (at stage i + 1's size)
  BlockBufs mid0, mid2;
  char* head_in;
  size_t state_total;
  // scratch
  char* x[SF_VAE_MAX_STAGES];      // the stage's running activation (residual blocks run in place)
  ResScratch rs;
  AttnScratch at;
  char* head_out;
  size_t scratch_total;
};

const sf_vae_resblock& res_at(const sf_vae_encoder* m, int stage, int j) { return m->res_host[stage * m->res_per_stage + j]; }

int stage_width(const sf_vae_encoder* m, int i) {   // widest activation of stage i (input and output of its blocks)
  int c = i == 0 ? m->in_conv.cout : 0;
  for (int j = 0; j < m->res_per_stage; ++j) {
    const sf_vae_resblock& r = res_at(m, i, j);
    c = std::max(c, std::max(r.conv1.cin, r.conv1.cout));
  }
  return c;
}

EPlan make_plan(const sf_vae_encoder* m, void* state, void* scratch, int H0, int W0, int K) {
  EPlan p;
  memset(&p, 0, sizeof(p));
  p.n_stages = m->n_stages;
  p.rps = m->res_per_stage;
  p.K = K;
  const int G = K - 1;            // chunks per call
  int T = 4;
  for (int i = 0; i < m->n_stages; ++i) {
    p.H[i] = H0 >> i;
    p.W[i] = W0 >> i;
    p.Tmax[i] = T;
    if (i + 1 < m->n_stages && m->temporal_down[i]) T /= 2;
  }
  const int L = m->n_stages - 1;
  const int Cm = m->mid0.conv1.cin;
  Carve st(state);
  p.c1_in = st.take(vol(hist_frames(K, p.Tmax[0]), p.H[0], p.W[0], m->in_conv.cin));
  for (int i = 0; i < m->n_stages; ++i) {
    for (int j = 0; j < m->res_per_stage; ++j) {
      const sf_vae_resblock& r = res_at(m, i, j);
      BlockBufs& b = p.blk[i * m->res_per_stage + j];
      b.a1 = st.take(vol(hist_frames(K, p.Tmax[i]), p.H[i], p.W[i], r.conv1.cin));
      b.a2 = st.take(vol(hist_frames(K, p.Tmax[i]), p.H[i], p.W[i], r.conv2.cin));
    }
    p.tc[i] = (i < L && m->time_conv[i].w) ? st.take(vol(hist_frames(K, p.Tmax[i]), p.H[i + 1], p.W[i + 1], m->time_conv[i].cin)) : nullptr;
  }
  p.mid0.a1 = st.take(vol(hist_frames(K, p.Tmax[L]), p.H[L], p.W[L], Cm)); p.mid0.a2 = st.take(vol(hist_frames(K, p.Tmax[L]), p.H[L], p.W[L], Cm));
  p.mid2.a1 = st.take(vol(hist_frames(K, p.Tmax[L]), p.H[L], p.W[L], Cm)); p.mid2.a2 = st.take(vol(hist_frames(K, p.Tmax[L]), p.H[L], p.W[L], Cm));
  p.head_in = st.take(vol(hist_frames(K, p.Tmax[L]), p.H[L], p.W[L], m->head_conv.cin));
  p.state_total = st.off;

  Carve sc(scratch);
  size_t y1_max = vol(G * p.Tmax[L], p.H[L], p.W[L], Cm), sc_max = 256;
  for (int i = 0; i < m->n_stages; ++i) {
    const int cw = std::max(stage_width(m, i), i == L ? Cm : 0);
    p.x[i] = sc.take(vol(G * p.Tmax[i], p.H[i], p.W[i], cw));
    for (int j = 0; j < m->res_per_stage; ++j) {
      const sf_vae_resblock& r = res_at(m, i, j);
      const size_t v = vol(G * p.Tmax[i], p.H[i], p.W[i], r.conv1.cout);
      if (v > y1_max) y1_max = v;
      if (r.shortcut.w && v > sc_max) sc_max = v;
    }
  }
  p.rs.y1 = sc.take(y1_max);
  p.rs.sc = sc.take(sc_max);
  const int n = p.H[L] * p.W[L];
  p.at.att_npad = (n + 63) & ~63;
  p.at.att_xn = sc.take((size_t)n * Cm * 2);
  p.at.att_qk = sc.take((size_t)n * 2 * Cm * 2);
  p.at.att_vt = sc.take((size_t)Cm * p.at.att_npad * 2);
  p.at.att_s = sc.take((size_t)n * p.at.att_npad * 4);
  p.at.att_p = sc.take((size_t)n * p.at.att_npad * 2);
  p.at.att_o = sc.take((size_t)n * Cm * 2);
  p.head_out = sc.take(vol(G * p.Tmax[L], p.H[L], p.W[L], m->head_conv.cout));
  p.scratch_total = sc.off;
  return p;
}

int check_encoder(const sf_vae_encoder* m, int H, int W, int K) {
  SF_CHECK(m != nullptr, "sf_vae_encode: null encoder");
  SF_CHECK(K >= 2 && K <= 64, "sf_vae_encode: window_frames %d (2..64: a call encodes up to window_frames - 1 chunks)", K);
  SF_CHECK(m->n_stages >= 2 && m->n_stages <= SF_VAE_MAX_STAGES && m->res_per_stage >= 1 && m->res_per_stage <= 8, "sf_vae_encode: bad stage counts");
  SF_CHECK(m->res_host && m->in_conv.w && m->head_conv.w && m->mid0.conv1.w && m->mid2.conv1.w && m->attn_qk_w && m->attn_v_w && m->attn_proj_w &&
           m->latent_mean && m->latent_std && m->conv1_w && m->conv1_b, "sf_vae_encode: encoder has null weights");
  int downs = 0;
  for (int i = 0; i + 1 < m->n_stages; ++i) {
    SF_CHECK(m->down_conv[i].w && m->down_conv[i].kh == 3 && m->down_conv[i].kt == 1, "sf_vae_encode: stage %d lacks its 3x3 stride-2 convolution", i);
    if (m->temporal_down[i]) {
      SF_CHECK(m->time_conv[i].w && m->time_conv[i].kt == 3 && m->time_conv[i].kh == 1, "sf_vae_encode: stage %d lacks its (3,1,1) time convolution", i);
      ++downs;
    }
  }
  SF_CHECK(downs == 2, "sf_vae_encode: %d temporal downsamplings (a chunk of 4 pixel frames must give one latent frame: 2)", downs);
  const int f = 1 << (m->n_stages - 1);
  SF_CHECK(H > 0 && W > 0 && H % f == 0 && W % f == 0, "sf_vae_encode: pixel size %dx%d must be a multiple of %d", H, W, f);
  SF_CHECK(((H / f) * (W / f)) % 4 == 0, "sf_vae_encode: latent size %dx%d (h*w must be a multiple of 4)", H / f, W / f);
  SF_CHECK(m->mid0.conv1.cin % 64 == 0, "sf_vae_encode: middle width %d must be a multiple of 64 (attention block GEMMs)", m->mid0.conv1.cin);
  SF_CHECK(m->in_conv.cin >= 8 && m->in_conv.cin % 8 == 0, "sf_vae_encode: encoder.conv1 input channels %d (3 padded to a multiple of 32)", m->in_conv.cin);
  SF_CHECK(m->z_dim > 0 && m->z_dim <= m->head_conv.cout && m->head_conv.cout <= 64, "sf_vae_encode: bad z_dim %d / head width %d", m->z_dim, m->head_conv.cout);
  return 0;
}

// every cached convolution's input volume: fn(buffer, frames per chunk at its stage, bytes per frame)
template <typename Fn>
int for_each_volume(const sf_vae_encoder* m, const EPlan& p, Fn fn) {
  const int L = m->n_stages - 1, Cm = m->mid0.conv1.cin;
  int rc = fn(p.c1_in, p.Tmax[0], vol(1, p.H[0], p.W[0], m->in_conv.cin));
  if (rc) return rc;
  for (int i = 0; i < m->n_stages; ++i) {
    for (int j = 0; j < m->res_per_stage; ++j) {
      const sf_vae_resblock& r = res_at(m, i, j);
      const BlockBufs& b = p.blk[i * m->res_per_stage + j];
      if ((rc = fn(b.a1, p.Tmax[i], vol(1, p.H[i], p.W[i], r.conv1.cin))) != 0) return rc;
      if ((rc = fn(b.a2, p.Tmax[i], vol(1, p.H[i], p.W[i], r.conv2.cin))) != 0) return rc;
    }
    if (p.tc[i] && (rc = fn(p.tc[i], p.Tmax[i], vol(1, p.H[i + 1], p.W[i + 1], m->time_conv[i].cin))) != 0) return rc;
  }
  char* mids[4] = {p.mid0.a1, p.mid0.a2, p.mid2.a1, p.mid2.a2};
  for (char* b : mids)
    if ((rc = fn(b, p.Tmax[L], vol(1, p.H[L], p.W[L], Cm))) != 0) return rc;
  return fn(p.head_in, p.Tmax[L], vol(1, p.H[L], p.W[L], m->head_conv.cin));
}

}  // namespace

extern "C" size_t sf_vae_encode_state_bytes(const sf_vae_encoder* m, int H, int W, int window_frames) {
  if (check_encoder(m, H, W, window_frames) != 0) return 0;
  return make_plan(m, nullptr, nullptr, H, W, window_frames).state_total;
}

extern "C" size_t sf_vae_encode_scratch_bytes(const sf_vae_encoder* m, int H, int W, int window_frames) {
  if (check_encoder(m, H, W, window_frames) != 0) return 0;
  return make_plan(m, nullptr, nullptr, H, W, window_frames).scratch_total;
}

extern "C" int sf_vae_encode_reset(const sf_vae_encoder* m, void* state, size_t state_bytes, int H, int W, int window_frames, void* stream) {
  SF_TRY(check_encoder(m, H, W, window_frames));
  const EPlan p = make_plan(m, state, nullptr, H, W, window_frames);
  SF_CHECK(state && state_bytes >= p.state_total, "sf_vae_encode_reset: state too small (%zu < %zu)", state_bytes, p.state_total);
  // as sf_vae_reset: only the two history frames at the front of every volume are read before they are written
  hipStream_t s = (hipStream_t)stream;
  return for_each_volume(m, p, [&](char* buf, int, size_t frame_bytes) -> int {
    return sf_hip_ok(hipMemsetAsync(buf, 0, 2 * frame_bytes, s), "sf_vae_encode_reset", "memset");
  });
}

extern "C" int sf_vae_encode_frames(const sf_vae_encoder* m, void* state, size_t state_bytes, void* scratch, size_t scratch_bytes,
                                    const void* pixels, int is_f32, int64_t c_stride, int H0, int W0, int window_frames, int chunk_index,
                                    int n_chunks, int window, int history_at, float* latents_out, void* stream) {
  SF_TRY(check_encoder(m, H0, W0, window_frames));
  SF_CHECK(pixels && latents_out, "sf_vae_encode_frames: null tensor");
  const int K = window_frames, G = n_chunks;
  SF_CHECK(chunk_index >= 0 && chunk_index < (1 << 24), "sf_vae_encode_frames: chunk_index %d (chunks encoded since the reset)", chunk_index);
  SF_CHECK(G >= 1 && G <= K - 1, "sf_vae_encode_frames: n_chunks %d (1..window_frames - 1 = %d)", G, K - 1);
  SF_CHECK(chunk_index > 0 || (G == 1 && window == 0 && history_at == 0),
           "sf_vae_encode_frames: the chunk that follows a reset is the first pixel frame, encoded alone at window 0 (vae.py:527-531)");
  SF_CHECK(window >= 0 && window + G <= K && window <= chunk_index, "sf_vae_encode_frames: window %d + %d chunks does not fit %d slots", window, G, K);
  SF_CHECK(history_at == window || (window == 0 && history_at >= 1 && history_at <= K && history_at <= chunk_index),
           "sf_vae_encode_frames: history_at %d (== window, or the previous lap's end when the window restarts at 0)", history_at);
  const Call cl = {chunk_index, G, window, history_at, (hipStream_t)stream};
  const bool first_chunk = cl.first_chunk();
  const EPlan p = make_plan(m, state, scratch, H0, W0, K);
  SF_CHECK(state && state_bytes >= p.state_total, "sf_vae_encode_frames: state too small (%zu < %zu)", state_bytes, p.state_total);
  SF_CHECK(scratch && scratch_bytes >= p.scratch_total, "sf_vae_encode_frames: scratch too small (%zu < %zu)", scratch_bytes, p.scratch_total);
  const int L = m->n_stages - 1;
  const int T0 = first_chunk ? 1 : 4 * G;
  SF_CHECK(c_stride >= (int64_t)T0 * H0 * W0, "sf_vae_encode_frames: channel stride %lld < %d frames of %dx%d", (long long)c_stride, T0, H0, W0);

  if (history_at != window)
    SF_TRY(for_each_volume(m, p, [&](char* buf, int Tmax, size_t frame_bytes) { return place_history(cl, buf, Tmax, frame_bytes); }));

  // pixels -> the new frames of encoder.conv1's input volume (3 channels padded to cin); conv1 (vae.py:324-336)
  const int c1 = cl.off(p.Tmax[0]);
  SF_TRY(sf_vae_prepare_pixels(pixels, is_f32, c_stride, p.c1_in + (size_t)(c1 + 2) * vol(1, H0, W0, m->in_conv.cin), T0, H0, W0, m->in_conv.cin, stream));
  SF_TRY(conv(m->in_conv, p.c1_in, T0, H0, W0, 0, c1, p.x[0], m->in_conv.cout, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream));

  // downsample stages (vae.py:339-343).  `normed`: the next block's conv1 input volume already holds SiLU(RMS_norm(cur))
  int T = T0;
  const char* cur = p.x[0];
  bool normed = false;
  for (int i = 0; i < m->n_stages; ++i) {
    const int H = p.H[i], W = p.W[i], Tmax = p.Tmax[i];
    SF_CHECK(T == (first_chunk ? 1 : G * Tmax), "sf_vae_encode_frames: stage %d expects %d frames, has %d", i, first_chunk ? 1 : G * Tmax, T);
    const int c_st = cl.off(Tmax);
    for (int j = 0; j < m->res_per_stage; ++j) {
      const sf_vae_resblock& r = res_at(m, i, j);
      NormOut next = {nullptr, nullptr, 0, 0};
      if (j + 1 < m->res_per_stage) {
        const sf_vae_resblock& rn = res_at(m, i, j + 1);
        next = {p.blk[i * m->res_per_stage + j + 1].a1, rn.gamma1, rn.conv1.cin, c_st + 2};
      }
      bool out_normed = false;
      SF_TRY(resblock(r, p.blk[i * m->res_per_stage + j], p.rs, cur, p.x[i], cl, T, Tmax, H, W, stream, normed, next.dst ? &next : nullptr, &out_normed));
      normed = out_normed;
      cur = p.x[i];
    }
    if (i == L) break;
    // Resample (vae.py:143-160): ZeroPad2d((0,1,0,1)) + Conv2d 3x3 stride 2 per frame
    const sf_vae_conv& dc = m->down_conv[i];
    const int Hn = p.H[i + 1], Wn = p.W[i + 1];
    if (m->temporal_down[i]) {
      // 'downsample3d': the spatial output is the time convolution's input (and, for the first chunk, the stage output
      // itself: no time convolution, the frame is the cache)
      const sf_vae_conv& tcv = m->time_conv[i];
      const int c_tc = cl.off(Tmax);
      char* tc_new = p.tc[i] + (size_t)(c_tc + 2) * vol(1, Hn, Wn, tcv.cin);
      SF_TRY(conv(dc, cur, T, Hn, Wn, 0, 0, tc_new, dc.cout, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream, nullptr, 2, 0));
      if (first_chunk) {
        cur = tc_new;
      } else {
        SF_TRY(conv(tcv, p.tc[i], T / 2, Hn, Wn, 0, c_tc + 1, p.x[i + 1], tcv.cout, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream, nullptr, 0, 2));
        cur = p.x[i + 1];
        T /= 2;
      }
    } else {
      SF_TRY(conv(dc, cur, T, Hn, Wn, 0, 0, p.x[i + 1], dc.cout, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream, nullptr, 2, 0));
      cur = p.x[i + 1];
    }
    normed = false;
  }

  // middle (vae.py:346-351): res, attention (per frame), res -- at the latent size
  const int h = p.H[L], w = p.W[L], Cm = m->mid0.conv1.cin;
  SF_CHECK(res_at(m, L, m->res_per_stage - 1).conv2.cout == Cm && m->mid0.conv1.cout == Cm && m->head_conv.cin == Cm,
           "sf_vae_encode_frames: the middle must keep the last stage's width");
  const AttnWeights aw = {m->attn_gamma, m->attn_qk_w, m->attn_qk_b, m->attn_v_w, m->attn_v_b, m->attn_proj_w, m->attn_proj_b};
  SF_TRY(resblock(m->mid0, p.mid0, p.rs, cur, p.x[L], cl, T, p.Tmax[L], h, w, stream));
  for (int f = 0; f < T; ++f) SF_TRY(attention_block(aw, p.at, p.x[L] + (size_t)f * vol(1, h, w, Cm), h * w, Cm, stream));
  SF_TRY(resblock(m->mid2, p.mid2, p.rs, p.x[L], p.x[L], cl, T, p.Tmax[L], h, w, stream));

  // head (vae.py:354-366): RMS-norm, SiLU, causal conv to 2 z_dim channels; then conv1 (mu rows) and the normalisation
  const int ch = cl.off(p.Tmax[L]);
  const int Ch = m->head_conv.cin, Co = m->head_conv.cout;
  SF_TRY(sf_rmsnorm_silu_cl(p.x[L], m->head_gamma, p.head_in + (size_t)(ch + 2) * vol(1, h, w, Ch), (long)T * h * w, Ch, 1, stream));
  SF_TRY(conv(m->head_conv, p.head_in, T, h, w, 0, ch, p.head_out, Co, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream));
  SF_TRY(sf_vae_finish_latent(p.head_out, Co, Co, m->conv1_w, Co, m->conv1_b, m->latent_mean, m->latent_std, latents_out, T, m->z_dim, h, w, stream));
  return 0;
}
