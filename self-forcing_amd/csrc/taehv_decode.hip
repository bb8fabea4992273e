// Host sequencer of the TAEHV tiny decoder (demo_utils/taehv.py:181-190 through apply_model_with_memblocks, :60-156)
// and its prepare kernel.  One call decodes a group of n latent frames into 4n pixel frames:
//
//   prepare (Clamp + layout)                                  [n][h][w][32]
//   decoder.1 + ReLU                                          -> block volume 0, behind its history frame
//   stage s = 0, 1, 2 (C = 256, 128, 64; T = n, n, 2n frames at h, 2h, 4h):
//     3 x MemBlock: conv.0 (kt = 2 over the block's volume: history frame + T new ones) + ReLU, conv.2 + ReLU,
//                   conv.4 + skip + ReLU written straight into the NEXT block's volume behind its history frame
//     exit: Upsample (read through the gather) + TGrow (folded into the weights; channel -> frame re-read in the
//           epilogue) + the bias-free 3x3 -> the next stage's first volume; the last exit also takes the ReLU behind it
//   decoder.22 (64 -> 3) with `* 2 - 1` and the clamp, planar float32
//
// Per-stream state = the one-frame history of each of the nine MemBlock input volumes; every volume lives in scratch.
// A call copies the histories to the front of the volumes, runs, and copies each volume's last frame back.
#include "sf_host.h"

namespace {

inline size_t vol(long T, int H, int W, int C) { return (size_t)T * H * W * C * 2; }

// geometry of stage s: channels, frame size, frames per latent frame
struct Stage { int C, H, W, T; };

int check_model(const sf_taehv_model* m, int lat_h, int lat_w, const char* who) {
  SF_CHECK(m != nullptr, "%s: null model", who);
  SF_CHECK(lat_h > 0 && lat_w > 0 && lat_h <= 4096 && lat_w <= 4096, "%s: latent size %dx%d", who, lat_h, lat_w);
  SF_CHECK(m->z_dim > 0 && m->z_dim <= m->in_conv.cin && m->in_conv.cin % 32 == 0 && m->in_conv.kt == 1 && m->in_conv.w && m->in_conv.bias,
           "%s: malformed input convolution", who);
  int c = m->in_conv.cout, tg = 1;
  for (int s = 0; s < SF_TAEHV_STAGES; ++s) {
    SF_CHECK(c > 0 && c % 32 == 0, "%s: stage %d has %d channels (a multiple of 32 expected)", who, s, c);
    for (int b = 0; b < SF_TAEHV_BLOCKS; ++b)
      for (int k = 0; k < 3; ++k) {
        const sf_taehv_layer& l = m->block[s][b][k];
        SF_CHECK(l.w && l.bias && l.cin == c && l.cout == c && l.kt == (k == 0 ? 2 : 1), "%s: malformed MemBlock %d.%d conv %d", who, s, b, k);
      }
    const sf_taehv_layer& e = m->exit_conv[s];
    SF_CHECK(m->tgrow[s] == 1 || m->tgrow[s] == 2, "%s: tgrow[%d] = %d (1 or 2)", who, s, m->tgrow[s]);
    SF_CHECK(e.w && e.cin == c && e.kt == 1 && e.cout > 0 && e.cout % (32 * m->tgrow[s]) == 0, "%s: malformed exit convolution of stage %d", who, s);
    c = e.cout / m->tgrow[s];
    tg *= m->tgrow[s];
  }
  SF_CHECK(tg == 4, "%s: the decoder must grow one latent frame into 4 frames", who);
  SF_CHECK(m->head.w && m->head.bias && m->head.cin == c && m->head.kt == 1 && m->head.cout == 3, "%s: malformed head", who);
  return 0;
}

void stages(const sf_taehv_model* m, int lat_h, int lat_w, Stage (&st)[SF_TAEHV_STAGES + 1]) {
  int c = m->in_conv.cout, h = lat_h, w = lat_w, t = 1;
  for (int s = 0; s <= SF_TAEHV_STAGES; ++s) {
    st[s] = {c, h, w, t};
    if (s < SF_TAEHV_STAGES) { c = m->exit_conv[s].cout / m->tgrow[s]; h *= 2; w *= 2; t *= m->tgrow[s]; }
  }
}

struct Bufs {
  char* x0;                                          // prepared latent [n][h][w][cin0]
  char* v[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];         // MemBlock input volumes: 1 history frame + n T frames
  char *ta, *tb, *tc;                                // conv.0 / conv.2 outputs, the stage's last MemBlock output
  char* head_in;                                     // [4n][8h][8w][64]
  size_t bytes;
};

Bufs carve_scratch(const sf_taehv_model* m, void* scratch, int lat_h, int lat_w, int n) {
  Stage st[SF_TAEHV_STAGES + 1];
  stages(m, lat_h, lat_w, st);
  Carve c(scratch);
  Bufs b;
  b.x0 = c.take(vol(n, lat_h, lat_w, m->in_conv.cin));
  size_t tmax = 0;
  for (int s = 0; s < SF_TAEHV_STAGES; ++s) {
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) b.v[s][k] = c.take(vol(1 + (long)n * st[s].T, st[s].H, st[s].W, st[s].C));
    const size_t t = vol((long)n * st[s].T, st[s].H, st[s].W, st[s].C);
    if (t > tmax) tmax = t;
  }
  b.ta = c.take(tmax); b.tb = c.take(tmax); b.tc = c.take(tmax);
  const Stage& l = st[SF_TAEHV_STAGES];
  b.head_in = c.take(vol((long)n * l.T, l.H, l.W, l.C));
  b.bytes = c.off;
  return b;
}

// offsets of the nine history frames inside the state block
size_t carve_state(const sf_taehv_model* m, void* state, int lat_h, int lat_w, char* (&hist)[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS]) {
  Stage st[SF_TAEHV_STAGES + 1];
  stages(m, lat_h, lat_w, st);
  Carve c(state);
  for (int s = 0; s < SF_TAEHV_STAGES; ++s)
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) hist[s][k] = c.take(vol(1, st[s].H, st[s].W, st[s].C));
  return c.off;
}

int conv(const sf_taehv_layer& l, const void* x, int Tout, int H, int W, int upsample, void* out, int ldo, int epi, const void* resid, int tgrow,
         float* out_f32, int clamp, void* stream) {
  sf_taehv_conv_args a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = l.w; a.bias = l.bias; a.out = out; a.resid = resid; a.out_f32 = out_f32;
  a.Tout = Tout; a.H = H; a.W = W; a.Cin = l.cin; a.Cout = l.cout; a.kt = l.kt; a.upsample = upsample;
  a.ldw = l.ldw; a.ldo = ldo; a.ldr = l.cout; a.tgrow = tgrow; a.epilogue = epi; a.clamp = clamp;
  return sf_taehv_conv(&a, stream);
}

__global__ __launch_bounds__(256) void taehv_prepare_kernel(const bf16_t* __restrict__ z, bf16_t* __restrict__ out, long n_pos, int hw, int zc, int c_pad) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (frame, position)
  if (i >= n_pos) return;
  const long f = i / hw, p = i - f * hw;
  const bf16_t* src = z + f * zc * hw + p;
  bf16_t* dst = out + i * c_pad;
  for (int c = 0; c < c_pad; c += 8) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c + j < zc ? (bf16_t)(3.0f * tanhf((float)src[(long)(c + j) * hw] * (1.0f / 3.0f))) : (bf16_t)0.f;
    *reinterpret_cast<bf16x8*>(dst + c) = v;
  }
}

}  // namespace

extern "C" int sf_taehv_prepare_latent(const void* latent, void* out, int n, int z, int h, int w, int c_pad, void* stream) {
  SF_CHECK(latent && out, "sf_taehv_prepare_latent: null tensor");
  SF_CHECK(n > 0 && z > 0 && h > 0 && w > 0 && c_pad >= z && c_pad % 8 == 0, "sf_taehv_prepare_latent: n=%d z=%d %dx%d c_pad=%d", n, z, h, w, c_pad);
  SF_CHECK((uintptr_t)out % 16 == 0, "sf_taehv_prepare_latent: misaligned output");
  const long n_pos = (long)n * h * w;
  return sf_launch<&taehv_prepare_kernel>("sf_taehv_prepare_latent", dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                          (const bf16_t*)latent, (bf16_t*)out, n_pos, h * w, z, c_pad);
}

extern "C" size_t sf_taehv_state_bytes(const sf_taehv_model* model, int lat_h, int lat_w) {
  if (check_model(model, lat_h, lat_w, "sf_taehv_state_bytes") != 0) return 0;
  char* hist[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];
  return carve_state(model, nullptr, lat_h, lat_w, hist);
}

extern "C" size_t sf_taehv_scratch_bytes(const sf_taehv_model* model, int lat_h, int lat_w, int max_frames) {
  if (check_model(model, lat_h, lat_w, "sf_taehv_scratch_bytes") != 0) return 0;
  if (max_frames < 1 || max_frames > 64) {
    sf_set_error("sf_taehv_scratch_bytes: max_frames=%d (1..64)", max_frames);
    return 0;
  }
  return carve_scratch(model, nullptr, lat_h, lat_w, max_frames).bytes;
}

extern "C" int sf_taehv_reset(const sf_taehv_model* model, void* state, size_t state_bytes, int lat_h, int lat_w, void* stream) {
  SF_TRY(check_model(model, lat_h, lat_w, "sf_taehv_reset"));
  SF_CHECK(state != nullptr, "sf_taehv_reset: null state");
  char* hist[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];
  const size_t need = carve_state(model, state, lat_h, lat_w, hist);
  SF_CHECK(state_bytes >= need, "sf_taehv_reset: state of %zu bytes, %zu needed", state_bytes, need);
  return sf_hip_ok(hipMemsetAsync(state, 0, need, (hipStream_t)stream), "sf_taehv_reset", "memset");
}

extern "C" int sf_taehv_decode_frames(const sf_taehv_model* model, void* state, size_t state_bytes, void* scratch, size_t scratch_bytes,
                                      const void* latent_frames, int lat_h, int lat_w, int n_frames, int clamp, float* pixels_out, void* stream) {
  SF_TRY(check_model(model, lat_h, lat_w, "sf_taehv_decode_frames"));
  SF_CHECK(state && scratch && latent_frames && pixels_out, "sf_taehv_decode_frames: null buffer");
  SF_CHECK(n_frames >= 1 && n_frames <= 64, "sf_taehv_decode_frames: n_frames=%d (1..64)", n_frames);
  SF_CHECK((uintptr_t)state % 256 == 0 && (uintptr_t)scratch % 256 == 0, "sf_taehv_decode_frames: state / scratch must be 256-byte aligned");
  char* hist[SF_TAEHV_STAGES][SF_TAEHV_BLOCKS];
  const size_t need_state = carve_state(model, state, lat_h, lat_w, hist);
  SF_CHECK(state_bytes >= need_state, "sf_taehv_decode_frames: state of %zu bytes, %zu needed", state_bytes, need_state);
  const Bufs b = carve_scratch(model, scratch, lat_h, lat_w, n_frames);
  SF_CHECK(scratch_bytes >= b.bytes, "sf_taehv_decode_frames: scratch of %zu bytes, %zu needed for %d frames", scratch_bytes, b.bytes, n_frames);
  Stage st[SF_TAEHV_STAGES + 1];
  stages(model, lat_h, lat_w, st);
  hipStream_t s = (hipStream_t)stream;
  const int n = n_frames;

  // the histories go to the front of their volumes
  for (int i = 0; i < SF_TAEHV_STAGES; ++i)
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k)
      SF_TRY(sf_hip_ok(hipMemcpyAsync(b.v[i][k], hist[i][k], vol(1, st[i].H, st[i].W, st[i].C), hipMemcpyDeviceToDevice, s), "sf_taehv_decode_frames",
                       "history copy"));
  SF_TRY(sf_taehv_prepare_latent(latent_frames, b.x0, n, model->z_dim, lat_h, lat_w, model->in_conv.cin, stream));
  SF_TRY(conv(model->in_conv, b.x0, n, lat_h, lat_w, 0, b.v[0][0] + vol(1, st[0].H, st[0].W, st[0].C), st[0].C, SF_TAEHV_BIAS_RELU, nullptr, 1, nullptr, 0,
              stream));
  for (int i = 0; i < SF_TAEHV_STAGES; ++i) {
    const Stage& g = st[i];
    const int T = n * g.T;
    const size_t f = vol(1, g.H, g.W, g.C);
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) {
      const sf_taehv_layer* l = model->block[i][k];
      char* x_new = b.v[i][k] + f;                                                       // the block's input, behind its history frame
      char* dst = k + 1 < SF_TAEHV_BLOCKS ? b.v[i][k + 1] + f : b.tc;
      SF_TRY(conv(l[0], b.v[i][k], T, g.H, g.W, 0, b.ta, g.C, SF_TAEHV_BIAS_RELU, nullptr, 1, nullptr, 0, stream));
      SF_TRY(conv(l[1], b.ta, T, g.H, g.W, 0, b.tb, g.C, SF_TAEHV_BIAS_RELU, nullptr, 1, nullptr, 0, stream));
      SF_TRY(conv(l[2], b.tb, T, g.H, g.W, 0, dst, g.C, SF_TAEHV_BIAS_RESID_RELU, x_new, 1, nullptr, 0, stream));
    }
    const Stage& nx = st[i + 1];
    const bool last = i + 1 == SF_TAEHV_STAGES;
    char* dst = last ? b.head_in : b.v[i + 1][0] + vol(1, nx.H, nx.W, nx.C);
    SF_TRY(conv(model->exit_conv[i], b.tc, T, nx.H, nx.W, 1, dst, nx.C, last ? SF_TAEHV_RELU : SF_TAEHV_PLAIN, nullptr, model->tgrow[i], nullptr, 0, stream));
  }
  const Stage& l = st[SF_TAEHV_STAGES];
  SF_TRY(conv(model->head, b.head_in, n * l.T, l.H, l.W, 0, nullptr, 0, SF_TAEHV_HEAD_F32, nullptr, 1, pixels_out, clamp, stream));
  // each volume's last frame is the next call's history
  for (int i = 0; i < SF_TAEHV_STAGES; ++i)
    for (int k = 0; k < SF_TAEHV_BLOCKS; ++k) {
      const size_t f = vol(1, st[i].H, st[i].W, st[i].C);
      SF_TRY(sf_hip_ok(hipMemcpyAsync(hist[i][k], b.v[i][k] + (size_t)n * st[i].T * f, f, hipMemcpyDeviceToDevice, s), "sf_taehv_decode_frames",
                       "history copy"));
    }
  return 0;
}
