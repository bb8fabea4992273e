// Host sequencer of the TAEHV tiny encoder (demo_utils/taehv.py:172-178 through apply_model_with_memblocks, :60-156).
// One call encodes n pixel frames (n % 4 == 0) into n / 4 latent frames:
//
//   encoder.0 + ReLU straight from the pixels (sf_taehv_encode_stem)     [n][H][W][64]
//   stage s = 0, 1, 2 (T = n/2, n/4, n/4 frames at H/2, H/4, H/8; 64 channels):
//     entry: TPool folded into the bias-free stride-2 3x3 (sf_taehv_down_conv, kt = 2, 2, 1) -> the stage's first
//            MemBlock volume, behind its history frame
//     3 x MemBlock: conv.0 (kt = 2 over the block's volume: history frame + T new ones) + ReLU, conv.2 + ReLU,
//                   conv.4 + skip + ReLU written straight into the NEXT block's volume behind its history frame
//   encoder.17 (64 -> 16) + bias, planar float32
//
// Per-stream state = the one-frame history of each of the nine MemBlock input volumes; every volume lives in scratch.
// A call copies the histories to the front of the volumes, runs, and copies each volume's last frame back.  A call
// carries whole groups of four frames, so no TPool ever waits for its second frame between calls.
#include "sf_host.h"

namespace {

inline size_t vol(long T, int H, int W, int C) { return (size_t)T * H * W * C * 2; }

// geometry of stage s for a call of n pixel frames: channels, frame size, frames
struct Stage { int C, H, W, T; };

int check_encoder(const sf_taehv_encoder* m, int H, int W, const char* who) {
  SF_CHECK(m != nullptr, "%s: null encoder", who);
  SF_CHECK(H > 0 && W > 0 && H <= 32768 && W <= 32768, "%s: frame size %dx%d", who, H, W);
  SF_CHECK(H % 8 == 0 && W % 8 == 0, "%s: height and width must be multiples of 8, got %dx%d", who, H, W);
  SF_CHECK(m->stem.w && m->stem.bias && m->stem.cin == 32 && m->stem.ldw == 32 && m->stem.cout == 64 && m->stem.kt == 1, "%s: malformed stem", who);
  int c = m->stem.cout, tf = 1;
  for (int s = 0; s < SF_TAEHV_STAGES; ++s) {
    const sf_taehv_layer& d = m->down[s];
    SF_CHECK(d.w && d.cin == c && d.cout > 0 && d.cout % 64 == 0 && (d.kt == 1 || d.kt == 2), "%s: malformed strided convolution of stage %d", who, s);
    c = d.cout;
    tf *= d.kt;
    for (int b = 0; b < SF_TAEHV_BLOCKS; ++b)
      for (int k = 0; k < 3; ++k) {
        const sf_taehv_layer& l = m->block[s][b][k];
        SF_CHECK(l.w && l.bias && l.cin == c && l.cout == c && l.kt == (k == 0 ? 2 : 1), "%s: malformed MemBlock %d.%d conv %d", who, s, b, k);
      }
  }
  SF_CHECK(tf == 4, "%s: the encoder must pool 4 frames into one latent frame", who);
  SF_CHECK(m->head.w && m->head.bias && m->head.cin == c && m->head.kt == 1 && m->head.cout > 0 && m->head.cout <= 32, "%s: malformed head", who);
  return 0;
}

void stages(const sf_taehv_encoder* m, int H, int W, int n, Stage (&st)[SF_TAEHV_STAGES]) {
  int h = H, w = W, t = n;
  for (int s = 0; s < SF_TAEHV_STAGES; ++s) {
    h /= 2; w /= 2; t /= m->down[s].kt;
    st[s] = {m->down[s].cout, h, w, t};
  }
}

struct Bufs {
  char* stem;                                        // [n][H][W][64]
  char* v[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];         // MemBlock input volumes: 1 history frame + T frames
  char *ta, *tb, *tc;                                // conv.0 / conv.2 outputs, the stage's last MemBlock output
  size_t bytes;
};

Bufs carve_scratch(const sf_taehv_encoder* m, void* scratch, int H, int W, int n) {
  Stage st[SF_TAEHV_STAGES];
  stages(m, H, W, n, st);
  Carve c(scratch);
  Bufs b;
  b.stem = c.take(vol(n, H, W, m->stem.cout));
  size_t tmax = 0;
  for (int s = 0; s < SF_TAEHV_STAGES; ++s) {
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) b.v[s][k] = c.take(vol(1 + (long)st[s].T, st[s].H, st[s].W, st[s].C));
    const size_t t = vol(st[s].T, st[s].H, st[s].W, st[s].C);
    if (t > tmax) tmax = t;
  }
  b.ta = c.take(tmax); b.tb = c.take(tmax); b.tc = c.take(tmax);
  b.bytes = c.off;
  return b;
}

// offsets of the nine history frames inside the state block
size_t carve_state(const sf_taehv_encoder* m, void* state, int H, int W, char* (&hist)[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS]) {
  Stage st[SF_TAEHV_STAGES];
  stages(m, H, W, 4, st);
  Carve c(state);
  for (int s = 0; s < SF_TAEHV_STAGES; ++s)
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) hist[s][k] = c.take(vol(1, st[s].H, st[s].W, st[s].C));
  return c.off;
}

int conv(const sf_taehv_layer& l, const void* x, int Tout, int H, int W, void* out, int epi, const void* resid, float* out_f32, void* stream) {
  sf_taehv_conv_args a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = l.w; a.bias = l.bias; a.out = out; a.resid = resid; a.out_f32 = out_f32;
  a.Tout = Tout; a.H = H; a.W = W; a.Cin = l.cin; a.Cout = l.cout; a.kt = l.kt;
  a.ldw = l.ldw; a.ldo = l.cout; a.ldr = l.cout; a.tgrow = 1; a.epilogue = epi;
  return sf_taehv_conv(&a, stream);
}

int down(const sf_taehv_layer& l, const void* x, int Tout, int H, int W, void* out, void* stream) {
  sf_taehv_down_conv_args a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = l.w; a.out = out;
  a.Tout = Tout; a.H = H; a.W = W; a.Cin = l.cin; a.Cout = l.cout; a.kt = l.kt; a.ldw = l.ldw; a.ldo = l.cout;
  return sf_taehv_down_conv(&a, stream);
}

}  // namespace

extern "C" size_t sf_taehv_encode_state_bytes(const sf_taehv_encoder* enc, int H, int W) {
  if (check_encoder(enc, H, W, "sf_taehv_encode_state_bytes") != 0) return 0;
  char* hist[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];
  return carve_state(enc, nullptr, H, W, hist);
}

extern "C" size_t sf_taehv_encode_scratch_bytes(const sf_taehv_encoder* enc, int H, int W, int max_frames) {
  if (check_encoder(enc, H, W, "sf_taehv_encode_scratch_bytes") != 0) return 0;
  if (max_frames < 4 || max_frames > 256 || max_frames % 4 != 0) {
    sf_set_error("sf_taehv_encode_scratch_bytes: max_frames=%d (a multiple of 4 in 4..256)", max_frames);
    return 0;
  }
  return carve_scratch(enc, nullptr, H, W, max_frames).bytes;
}

extern "C" int sf_taehv_encode_reset(const sf_taehv_encoder* enc, void* state, size_t state_bytes, int H, int W, void* stream) {
  SF_TRY(check_encoder(enc, H, W, "sf_taehv_encode_reset"));
  SF_CHECK(state != nullptr, "sf_taehv_encode_reset: null state");
  char* hist[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];
  const size_t need = carve_state(enc, state, H, W, hist);
  SF_CHECK(state_bytes >= need, "sf_taehv_encode_reset: state of %zu bytes, %zu needed", state_bytes, need);
  return sf_hip_ok(hipMemsetAsync(state, 0, need, (hipStream_t)stream), "sf_taehv_encode_reset", "memset");
}

extern "C" int sf_taehv_encode_frames(const sf_taehv_encoder* enc, void* state, size_t state_bytes, void* scratch, size_t scratch_bytes, const void* pixels,
                                      int dtype, int64_t c_stride, int H, int W, int n_frames, int lead, float* latents_out, void* stream) {
  SF_TRY(check_encoder(enc, H, W, "sf_taehv_encode_frames"));
  SF_CHECK(state && scratch && pixels && latents_out, "sf_taehv_encode_frames: null buffer");
  SF_CHECK(n_frames >= 4 && n_frames <= 256 && n_frames % 4 == 0, "sf_taehv_encode_frames: n_frames=%d must be a multiple of 4 in 4..256", n_frames);
  SF_CHECK(lead >= 0 && lead <= 3, "sf_taehv_encode_frames: lead=%d (0..3)", lead);
  SF_CHECK((uintptr_t)state % 256 == 0 && (uintptr_t)scratch % 256 == 0, "sf_taehv_encode_frames: state / scratch must be 256-byte aligned");
  char* hist[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];
  const size_t need_state = carve_state(enc, state, H, W, hist);
  SF_CHECK(state_bytes >= need_state, "sf_taehv_encode_frames: state of %zu bytes, %zu needed", state_bytes, need_state);
  const Bufs b = carve_scratch(enc, scratch, H, W, n_frames);
  SF_CHECK(scratch_bytes >= b.bytes, "sf_taehv_encode_frames: scratch of %zu bytes, %zu needed for %d frames", scratch_bytes, b.bytes, n_frames);
  Stage st[SF_TAEHV_STAGES];
  stages(enc, H, W, n_frames, st);
  hipStream_t s = (hipStream_t)stream;

  // the histories go to the front of their volumes
  for (int i = 0; i < SF_TAEHV_STAGES; ++i)
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k)
      SF_TRY(sf_hip_ok(hipMemcpyAsync(b.v[i][k], hist[i][k], vol(1, st[i].H, st[i].W, st[i].C), hipMemcpyDeviceToDevice, s), "sf_taehv_encode_frames",
                       "history copy"));
  SF_TRY(sf_taehv_encode_stem(pixels, dtype, c_stride, H, W, n_frames, lead, enc->stem.w, enc->stem.bias, b.stem, stream));
  const char* src = b.stem;
  for (int i = 0; i < SF_TAEHV_STAGES; ++i) {
    const Stage& g = st[i];
    const size_t f = vol(1, g.H, g.W, g.C);
    SF_TRY(down(enc->down[i], src, g.T, g.H, g.W, b.v[i][0] + f, stream));
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) {
      const sf_taehv_layer* l = enc->block[i][k];
      char* x_new = b.v[i][k] + f;                                                       // the block's input, behind its history frame
      char* dst = k + 1 < SF_TAEHV_BLOCKS ? b.v[i][k + 1] + f : b.tc;
      SF_TRY(conv(l[0], b.v[i][k], g.T, g.H, g.W, b.ta, SF_TAEHV_BIAS_RELU, nullptr, nullptr, stream));
      SF_TRY(conv(l[1], b.ta, g.T, g.H, g.W, b.tb, SF_TAEHV_BIAS_RELU, nullptr, nullptr, stream));
      SF_TRY(conv(l[2], b.tb, g.T, g.H, g.W, dst, SF_TAEHV_BIAS_RESID_RELU, x_new, nullptr, stream));
    }
    src = b.tc;
  }
  const Stage& l = st[SF_TAEHV_STAGES - 1];
  SF_TRY(conv(enc->head, b.tc, l.T, l.H, l.W, nullptr, SF_TAEHV_LATENT_F32, nullptr, latents_out, stream));
  // each volume's last frame is the next call's history
  for (int i = 0; i < SF_TAEHV_STAGES; ++i)
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) {
      const size_t f = vol(1, st[i].H, st[i].W, st[i].C);
      SF_TRY(sf_hip_ok(hipMemcpyAsync(hist[i][k], b.v[i][k] + (size_t)st[i].T * f, f, hipMemcpyDeviceToDevice, s), "sf_taehv_encode_frames", "history copy"));
    }
  return 0;
}
