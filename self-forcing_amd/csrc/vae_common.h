// Internal helpers shared by the VAE decode (vae_decode.hip) and encode (vae_encode.hip) sequencers: the carving of the
// state / scratch blocks, the sliding history windows of the cached convolutions' input volumes, and the host-side
// composition of ResidualBlock (vae.py:182-221) and AttentionBlock (vae.py:223-264) from the library's kernels.
// Host-side only.  Both sequencers enqueue exactly these calls, so the decoder's arithmetic is unchanged by the sharing.
#pragma once
#include <cmath>
#include "sf_host.h"

namespace sfvae {

struct BlockBufs { char *a1, *a2; };   // the two cached input volumes of a ResidualBlock (conv1's, conv2's)
struct ResScratch { char *y1, *sc; };   // conv1's raw output (when its norm is not fused), the shortcut's output
struct AttnScratch { char *att_xn, *att_qk, *att_vt, *att_s, *att_p, *att_o; int att_npad; };
struct AttnWeights {                     // AttentionBlock: norm gamma, to_qkv split into q|k and v rows, proj
  const void* attn_gamma;
  const void *attn_qk_w, *attn_qk_b, *attn_v_w, *attn_v_b, *attn_proj_w, *attn_proj_b;
};

inline size_t vol(int T, int H, int W, int C) { return (size_t)T * H * W * C * 2; }

// Sliding history window of a cached convolution's input volume (capacity 2 + K * Tmax frames, K latent frames).
// A lap = the calls between two restarts at slot 0; slot q of a lap holds the frames of the lap's q-th latent frame.
// The lap that begins at the reset is special: its slot 0 is the first chunk, which has ONE frame at every stage
// (vae.py:109-111) and never enters a time convolution's volume (the quirk of vae.py:104-132).
inline int hist_frames(int K, int Tmax) { return 2 + K * Tmax; }
inline int vol_off(int lap_start, int slot, int Tmax, bool time_conv) {   // first history frame of the window that starts at `slot`
  if (lap_start != 0 || slot == 0) return slot * Tmax;
  return time_conv ? (slot - 1) * Tmax : 1 + (slot - 1) * Tmax;
}

struct Call {                 // one sf_vae_decode_frames / sf_vae_encode_frames call (n: latent frames / chunks since the reset)
  int n, F, window, history_at;
  hipStream_t s;
  bool first_chunk() const { return n == 0; }
  int off(int Tmax, bool tc = false) const { return vol_off(n - window, window, Tmax, tc); }
};

// the two history frames of a volume are where the previous call left them (slot `history_at` of ITS lap); a call that
// restarts the window copies them to the front first (frame by frame: the ranges may overlap by one frame)
inline int place_history(const Call& c, char* buf, int Tmax, size_t frame_bytes, bool tc = false) {
  if (c.history_at == c.window) return 0;
  if (tc && c.n - c.history_at == 0 && c.history_at <= 1) return 0;   // only the first chunk so far: this volume is still all zero
  const int src = vol_off(c.n - c.history_at, c.history_at, Tmax, tc), dst = c.off(Tmax, tc);
  for (int k = 0; k < 2; ++k)
    SF_TRY(sf_hip_ok(hipMemcpyAsync(buf + (size_t)(dst + k) * frame_bytes, buf + (size_t)(src + k) * frame_bytes, frame_bytes, hipMemcpyDeviceToDevice, c.s),
                     "sf_vae", "history copy"));
  return 0;
}

// RMS_norm + SiLU of a convolution's output can ride in its epilogue (second output of the halo kernel) when the
// convolution is 3 x 3 spatial with 96 or 192 output channels at a resolution the halo kernel takes
struct NormOut { void* dst; const void* gamma; int ld; int frame_off; };   // dst: base of the consumer's input volume; its new frames start at frame_off

inline bool can_fuse_norm(const sf_vae_conv& c, int H, int W) { return c.kh == 3 && c.kw == 3 && (c.cout == 96 || c.cout == 192) && H >= 16 && W >= 16; }

// `stride` = 2: the encoder's downsampling -- Conv2d 3x3 stride 2 behind ZeroPad2d((0,1,0,1)) (input 2H x 2W) and / or
// the (3,1,1) time convolution with temporal stride 2 (sf_conv_args.stride_hw / stride_t)
inline int conv(const sf_vae_conv& c, const void* x, int Tout, int H, int W, int upsample, int t_off, void* out, int ldo, int out_frame0,
         int interleave_c, int epi, const void* resid, int ldr, float* out_f32, void* stream, const NormOut* norm = nullptr,
         int stride_hw = 0, int stride_t = 0) {
  sf_conv_args a;
  memset(&a, 0, sizeof(a));
  if (norm) { a.norm_out = norm->dst; a.norm_gamma = norm->gamma; a.norm_ld = norm->ld; a.norm_frame_offset = norm->frame_off; }
  a.x = x; a.w = c.w; a.bias = c.bias; a.out = out; a.resid = resid; a.out_f32 = out_f32;
  a.Tout = Tout; a.H = H; a.W = W; a.Hin = upsample ? H / 2 : stride_hw == 2 ? 2 * H : H; a.Win = upsample ? W / 2 : stride_hw == 2 ? 2 * W : W;
  a.Cin = c.cin; a.Cout = c.cout; a.kt = c.kt; a.kh = c.kh; a.kw = c.kw; a.upsample = upsample; a.t_in_offset = t_off;
  a.ldw = c.ldw; a.ldo = ldo; a.ldr = ldr; a.out_frame_offset = out_frame0; a.interleave_c = interleave_c; a.epilogue = epi;
  a.stride_hw = stride_hw; a.stride_t = stride_t;
  return sf_conv_igemm(&a, stream);
}

// ResidualBlock.forward (vae.py:202-221) on T frames of H x W.  `in_normed`: the producer of x_in already wrote
// SiLU(RMS_norm(x_in)) into conv1's input volume (fused epilogue); `next`: where (and with which gamma) this block's
// output should ALSO be written normalised -- the next block's conv1 input or the head's --, if its conv2 can do that.
// Returns through *out_normed whether it did.
inline int resblock(const sf_vae_resblock& r, const BlockBufs& b, const ResScratch& p, const char* x_in, char* out, const Call& cl, int T, int Tmax, int H, int W,
             void* stream, bool in_normed = false, const NormOut* next = nullptr, bool* out_normed = nullptr) {
  const long rows = (long)T * H * W;
  const int cin = r.conv1.cin, cout = r.conv1.cout;
  const size_t f1 = vol(1, H, W, cin), f2 = vol(1, H, W, cout);
  const int c = cl.off(Tmax);                         // both volumes of the block slide alike
  if (!in_normed) SF_TRY(sf_rmsnorm_silu_cl(x_in, r.gamma1, b.a1 + (size_t)(c + 2) * f1, rows, cin, 1, stream));
  if (can_fuse_norm(r.conv1, H, W)) {   // conv1's raw output is only ever read by the norm in front of conv2
    const NormOut n2 = {b.a2, r.gamma2, cout, c + 2};
    SF_TRY(conv(r.conv1, b.a1, T, H, W, 0, c, nullptr, cout, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream, &n2));
  } else {
    SF_TRY(conv(r.conv1, b.a1, T, H, W, 0, c, p.y1, cout, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream));
    SF_TRY(sf_rmsnorm_silu_cl(p.y1, r.gamma2, b.a2 + (size_t)(c + 2) * f2, rows, cout, 1, stream));
  }
  const char* resid = x_in;
  if (r.shortcut.w) {
    SF_TRY(conv(r.shortcut, x_in, T, H, W, 0, 0, p.sc, cout, 0, 0, SF_CONV_BIAS, nullptr, 0, nullptr, stream));
    resid = p.sc;
  }
  const bool fuse_next = next && next->ld == r.conv2.cout && can_fuse_norm(r.conv2, H, W);
  SF_TRY(conv(r.conv2, b.a2, T, H, W, 0, c, out, cout, 0, 0, SF_CONV_BIAS_RESID, resid, cout, nullptr, stream, fuse_next ? next : nullptr));
  if (out_normed) *out_normed = fuse_next;
  return 0;
}

// AttentionBlock.forward (vae.py:241-264) on one frame of n = h*w positions, in place on x [n][C]
inline int attention_block(const AttnWeights& m, const AttnScratch& p, char* x, int n, int C, void* stream) {
  const int np = p.att_npad;
  SF_TRY(sf_rmsnorm_silu_cl(x, m.attn_gamma, p.att_xn, n, C, 0, stream));
  SF_TRY(Gemm(p.att_xn, C, m.attn_qk_w, C, p.att_qk, 2 * C, n, 2 * C, C).bias(m.attn_qk_b).bf16(stream));
  // V^T [C][np] = Wv . xn^T straight from the projection (no transpose pass); its bias is added after
  // the P.V product instead (softmax rows sum to one), the padded key columns stay zero
  SF_TRY(sf_hip_ok(hipMemsetAsync(p.att_vt, 0, (size_t)C * np * 2, (hipStream_t)stream), "sf_vae", "memset"));
  SF_TRY(Gemm(m.attn_v_w, C, p.att_xn, C, p.att_vt, np, C, n, C).bf16(stream));
  SF_TRY(Gemm(p.att_qk, 2 * C, p.att_qk + (size_t)C * 2, 2 * C, p.att_s, np, n, n, C).epi(SF_EPI_F32).bf16(stream));
  SF_TRY(sf_softmax_rows((const float*)p.att_s, np, p.att_p, np, n, n, np, 1.0f / sqrtf((float)C), stream));
  SF_TRY(Gemm(p.att_p, np, p.att_vt, np, p.att_o, C, n, C, np).bias(m.attn_v_b).bf16(stream));
  SF_TRY(Gemm(p.att_o, C, m.attn_proj_w, C, x, C, n, C, C).bias(m.attn_proj_b).epi(SF_EPI_BIAS_RESID).resid(x, C).bf16(stream));
  return 0;
}


}  // namespace sfvae
