// Host sequencer of the pose front end (pipeline/causal_diffusion_inference.py:87-122, :337-343) and the gather in
// front of its last layer.  One call embeds a whole clip:
//
//   prepare (first frame x3 in front, / 255, layout)          [F+3][H][W][8]
//   dwpose_embedding.0 .. .10: six sf_pose_conv with SiLU     -> [F'][2h][2w][16]   (two ping-pong volumes)
//   dwpose_embedding.12 (16 -> 5120, kernel = stride = (1,2,2)): the patch-embed pattern -- gather each token's 2x2x16
//     patch into a row of [F'*h*w][64], then sf_gemm_bf16 with the bias epilogue -> tokens [F'*h*w][5120], token-major
//
// and the reference-pose stack is six sf_pose_conv with kt = 1 on one image.  Everything lives in scratch; the library
// keeps no state.  The same dwpose stack also runs piece by piece (sf_pose_stream_push, at the end of this file): every
// layer over a temporal window of its input (sf_pose_conv_window), two frames of history per layer input in a buffer
// the caller owns, the bits of the whole clip.
#include "sf_host.h"

namespace {

constexpr long VOL_LIMIT = 0xFFFFFF00L;   // sf_pose_conv's 32-bit byte offsets

struct Vol { int T, H, W, C; };
inline size_t vbytes(const Vol& v) { return (size_t)v.T * v.H * v.W * v.C * 2; }

int check_layers(const sf_pose_layer* l, int kt, const char* who, const char* stack) {
  int c = 8;
  for (int i = 0; i < SF_POSE_CONVS; ++i) {
    SF_CHECK(l[i].w && l[i].bias, "%s: %s layer %d has no weights", who, stack, i);
    SF_CHECK(l[i].cin == c && l[i].kt == kt && l[i].cout > 0 && l[i].cout <= 32, "%s: malformed %s layer %d (cin=%d cout=%d kt=%d)", who, stack, i,
             l[i].cin, l[i].cout, l[i].kt);
    SF_CHECK(i + 1 == SF_POSE_CONVS || l[i].cout == 16, "%s: %s layer %d must have 16 output channels", who, stack, i);
    SF_CHECK((l[i].stride_t == 1 || l[i].stride_t == 2) && (l[i].stride_s == 1 || l[i].stride_s == 2), "%s: %s layer %d has strides (%d, %d)", who, stack,
             i, l[i].stride_t, l[i].stride_s);
    c = 16;
  }
  return 0;
}

int check_model(const sf_pose_model* m, int F, int H, int W, const char* who) {
  SF_CHECK(m != nullptr, "%s: null model", who);
  SF_CHECK(F >= 0 && F <= (1 << 20) && H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16), "%s: F=%d H=%d W=%d", who, F, H, W);
  if (F > 0) {
    SF_TRY(check_layers(m->conv, 3, who, "dwpose"));
    SF_CHECK(m->conv[SF_POSE_CONVS - 1].cout == 16, "%s: the last dwpose convolution must have 16 output channels", who);
    SF_CHECK(m->embed_w && m->embed_b && m->pose_dim > 0 && m->pose_dim % 4 == 0, "%s: malformed token embedding (pose_dim=%d)", who, m->pose_dim);
  } else {
    SF_TRY(check_layers(m->ref_conv, 1, who, "reference-pose"));
  }
  return 0;
}

// The volumes of a stack: v[0] the prepared input, v[i + 1] the output of layer i.  -1 when one reaches 4 GiB.
int plan(const sf_pose_layer* l, int T, int H, int W, Vol (&v)[SF_POSE_CONVS + 1], int last_ld, const char* who) {
  v[0] = {T, H, W, 8};
  for (int i = 0; i < SF_POSE_CONVS; ++i) {
    const Vol& a = v[i];
    v[i + 1] = {l[i].kt == 3 ? sf_pose_out_size(a.T, 3, l[i].stride_t) : a.T, sf_pose_out_size(a.H, 3, l[i].stride_s),
                sf_pose_out_size(a.W, 3, l[i].stride_s), i + 1 == SF_POSE_CONVS ? last_ld : 16};
  }
  for (int i = 0; i <= SF_POSE_CONVS; ++i) {
    const long b = (long)v[i].T * v[i].H * v[i].W * v[i].C * 2;
    SF_CHECK(b < VOL_LIMIT, "%s: a %dx%dx%d volume of %d channels is %ld bytes, beyond the 4 GiB the convolution's 32-bit offsets cover; embed the clip "
             "in shorter pieces or at a lower resolution", who, v[i].T, v[i].H, v[i].W, v[i].C, b);
  }
  return 0;
}

struct Bufs { char *in, *a, *b, *rows; size_t bytes; };

// in: the prepared volume; a / b: ping-pong for the layer outputs (a takes layers 0, 2, 4; b layers 1, 3, 5);
// rows: the gathered [tokens][64] rows of the token embedding (dwpose stack only)
Bufs carve(void* scratch, const Vol (&v)[SF_POSE_CONVS + 1], long tokens) {
  size_t sa = 0, sb = 0;
  for (int i = 0; i < SF_POSE_CONVS; ++i) {
    size_t& s = (i & 1) ? sb : sa;
    if (vbytes(v[i + 1]) > s) s = vbytes(v[i + 1]);
  }
  Bufs r;
  Carve c(scratch);
  r.in = c.take(vbytes(v[0]));
  r.a = c.take(sa);
  r.b = c.take(sb);
  r.rows = c.take((size_t)tokens * 64 * 2);
  r.bytes = c.off;
  return r;
}

int run_stack(const sf_pose_layer* l, const Vol (&v)[SF_POSE_CONVS + 1], const Bufs& b, void* last_out, void* stream) {
  const char* x = b.in;
  for (int i = 0; i < SF_POSE_CONVS; ++i) {
    char* out = i + 1 == SF_POSE_CONVS && last_out ? (char*)last_out : (i & 1) ? b.b : b.a;
    sf_pose_conv_args a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = l[i].w; a.bias = l[i].bias; a.out = out;
    a.T = v[i].T; a.H = v[i].H; a.W = v[i].W; a.Cin = l[i].cin; a.Cout = l[i].cout;
    a.kt = l[i].kt; a.stride_t = l[i].stride_t; a.stride_s = l[i].stride_s; a.ldw = l[i].ldw; a.ldo = v[i + 1].C; a.silu = l[i].silu;
    SF_TRY(sf_pose_conv(&a, stream));
    x = out;
  }
  return 0;
}

// rows[(f, i, j)][(dh*2 + dw)*16 + c] = x[f][2i + dh][2j + dw][c]: one 16-byte piece per thread
__global__ __launch_bounds__(256) void pose_patch_gather_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ rows, long n_pieces, int H, int W, int h,
                                                                int w) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pieces) return;
  const long m = i >> 3;
  const int q = (int)(i & 7), tap = q >> 1, half = q & 1;
  const long f = m / (h * w);
  const int r = (int)(m - f * (h * w)), ii = r / w, jj = r - ii * w;
  const long src = ((f * H + 2 * ii + (tap >> 1)) * W + 2 * jj + (tap & 1)) * 16 + half * 8;
  *reinterpret_cast<bf16x8*>(rows + i * 8) = *reinterpret_cast<const bf16x8*>(x + src);
}

}  // namespace

extern "C" int sf_pose_patch_embed(const void* x, int T, int H, int W, const void* w, const void* bias, int pose_dim, void* rows, void* tokens_out,
                                   void* stream) {
  const char* who = "sf_pose_patch_embed";
  SF_CHECK(x && w && bias && rows && tokens_out, "%s: null tensor", who);
  SF_CHECK(T > 0 && H >= 2 && W >= 2 && H <= (1 << 16) && W <= (1 << 16) && pose_dim > 0 && pose_dim % 4 == 0, "%s: T=%d H=%d W=%d pose_dim=%d", who, T, H, W,
           pose_dim);
  SF_CHECK((uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)rows % 16 == 0 && (uintptr_t)tokens_out % 16 == 0, "%s: misaligned tensor", who);
  const int h = H / 2, wd = W / 2;
  const long tokens = (long)T * h * wd;
  SF_CHECK(tokens < (1L << 31) / 8, "%s: %ld tokens", who, tokens);
  const long n_pieces = tokens * 8;
  SF_TRY(sf_launch<&pose_patch_gather_kernel>(who, dim3((unsigned)((n_pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)rows,
                                              n_pieces, H, W, h, wd));
  return Gemm(rows, 64, w, 64, tokens_out, pose_dim, (int)tokens, pose_dim, 64).bias(bias).bf16(stream);
}

extern "C" size_t sf_pose_scratch_bytes(const sf_pose_model* model, int F, int H, int W) {
  const char* who = "sf_pose_scratch_bytes";
  if (check_model(model, F, H, W, who) != 0) return 0;
  Vol v[SF_POSE_CONVS + 1];
  if (F > 0) {
    if (plan(model->conv, F + 3, H, W, v, 16, who) != 0) return 0;
    const Vol& l = v[SF_POSE_CONVS];
    const long tokens = (long)l.T * sf_pose_out_size(l.H, 2, 2) * sf_pose_out_size(l.W, 2, 2);
    if (tokens <= 0) {
      sf_set_error("%s: %d frames of %dx%d give no tokens", who, F, H, W);
      return 0;
    }
    return carve(nullptr, v, tokens).bytes;
  }
  if (plan(model->ref_conv, 1, H, W, v, model->ref_conv[SF_POSE_CONVS - 1].cout, who) != 0) return 0;
  return carve(nullptr, v, 0).bytes;
}

extern "C" int sf_pose_embed(const sf_pose_model* model, const void* frames, int dtype, int F, int H, int W, void* scratch, size_t scratch_bytes,
                             void* tokens_out, int64_t n_tokens, void* stream) {
  const char* who = "sf_pose_embed";
  SF_TRY(check_model(model, F, H, W, who));
  SF_CHECK(F >= 1, "%s: no frames", who);
  SF_CHECK(frames && scratch && tokens_out, "%s: null buffer", who);
  SF_CHECK(dtype >= SF_POSE_U8 && dtype <= SF_POSE_BF16, "%s: unknown dtype %d", who, dtype);
  SF_CHECK((uintptr_t)scratch % 256 == 0 && (uintptr_t)tokens_out % 16 == 0, "%s: scratch must be 256-byte, tokens_out 16-byte aligned", who);
  Vol v[SF_POSE_CONVS + 1];
  SF_TRY(plan(model->conv, F + 3, H, W, v, 16, who));
  const Vol& l = v[SF_POSE_CONVS];
  const int h = sf_pose_out_size(l.H, 2, 2), w = sf_pose_out_size(l.W, 2, 2);
  const long tokens = (long)l.T * h * w;
  SF_CHECK(tokens > 0 && tokens < (1L << 31) / 8, "%s: %d frames of %dx%d give %ld tokens", who, F, H, W, tokens);
  SF_CHECK(n_tokens == tokens, "%s: tokens_out holds %ld rows, %d frames of %dx%d give %d x %d x %d = %ld", who, (long)n_tokens, F, H, W, l.T, h, w, tokens);
  const Bufs b = carve(scratch, v, tokens);
  SF_CHECK(scratch_bytes >= b.bytes, "%s: scratch of %zu bytes, %zu needed", who, scratch_bytes, b.bytes);

  SF_TRY(sf_pose_prepare(frames, dtype, 0, F, H, W, 3, b.in, stream));
  SF_TRY(run_stack(model->conv, v, b, nullptr, stream));
  const char* x = ((SF_POSE_CONVS - 1) & 1) ? b.b : b.a;
  return sf_pose_patch_embed(x, l.T, l.H, l.W, model->embed_w, model->embed_b, model->pose_dim, b.rows, tokens_out, stream);
}

extern "C" int sf_pose_embed_ref(const sf_pose_model* model, const void* image, int dtype, int H, int W, void* scratch, size_t scratch_bytes, void* out,
                                 void* stream) {
  const char* who = "sf_pose_embed_ref";
  SF_TRY(check_model(model, 0, H, W, who));
  SF_CHECK(image && scratch && out, "%s: null buffer", who);
  SF_CHECK(dtype >= SF_POSE_U8 && dtype <= SF_POSE_BF16, "%s: unknown dtype %d", who, dtype);
  SF_CHECK((uintptr_t)scratch % 256 == 0 && (uintptr_t)out % 8 == 0, "%s: scratch must be 256-byte, out 8-byte aligned", who);
  Vol v[SF_POSE_CONVS + 1];
  SF_TRY(plan(model->ref_conv, 1, H, W, v, model->ref_conv[SF_POSE_CONVS - 1].cout, who));
  const Bufs b = carve(scratch, v, 0);
  SF_CHECK(scratch_bytes >= b.bytes, "%s: scratch of %zu bytes, %zu needed", who, scratch_bytes, b.bytes);
  SF_TRY(sf_pose_prepare(image, dtype, 1, 1, H, W, 0, b.in, stream));
  return run_stack(model->ref_conv, v, b, out, stream);
}

// ------------------------------------------------------------------------------------------------ the resumable stack
// A clip pushed piece by piece.  Level 0 is the prepared volume, level i + 1 the output of convolution i; the temporal
// strides are the dwpose stack's (1, 1, 1, 1, 2, 2).  A layer's output frame t reads input frames t*st - 1 .. t*st + 1, so
// with N final input frames of an open clip a stride-1 layer has N - 1 final output frames and a stride-2 layer N / 2;
// once the clip is closed every level is complete.  A push computes, level by level, the frames between the old and the
// new frontier; the lowest input frame they read is never more than two behind the input's old frontier, so two frames
// of history per layer input (the caller's `state`) carry everything, and a window of 2 + new frames holds every tap.
namespace {

constexpr int POSE_STREAM_ST[SF_POSE_CONVS] = {1, 1, 1, 1, 2, 2};
constexpr int STREAM_MAX_FRAMES = 1 << 28;

// final frames of every level with P pixel frames known
void stream_frontier(int P, bool closed, int (&f)[SF_POSE_LEVELS]) {
  f[0] = P > 0 ? P + 3 : 0;
  for (int i = 0; i < SF_POSE_CONVS; ++i) {
    const int n = f[i], st = POSE_STREAM_ST[i];
    f[i + 1] = n <= 0 ? 0 : closed ? sf_pose_out_size(n, 3, st) : st == 1 ? n - 1 : n / 2;
  }
}

// the most frames level l gains in one push of n pixel frames, first, middle or closing (the host test walks it)
inline int stream_cap(int l, int n) { return l <= 4 ? n + 4 : l == 5 ? (n + 3) / 2 + 2 : (n + 3) / 4 + 2; }

struct StreamGeo {
  Vol v[SF_POSE_LEVELS];          // T = 1: one frame of each level
  size_t frame[SF_POSE_LEVELS];   // its bytes
  int h, w;                       // tokens per latent frame: h x w
};

int stream_geo(const sf_pose_model* m, int H, int W, StreamGeo& g, const char* who) {
  SF_TRY(check_model(m, 1, H, W, who));
  for (int i = 0; i < SF_POSE_CONVS; ++i)
    SF_CHECK(m->conv[i].stride_t == POSE_STREAM_ST[i], "%s: dwpose layer %d has temporal stride %d, the streamed stack expects %d", who, i,
             m->conv[i].stride_t, POSE_STREAM_ST[i]);
  SF_TRY(plan(m->conv, 1, H, W, g.v, 16, who));
  for (int l = 0; l < SF_POSE_LEVELS; ++l) g.frame[l] = vbytes(g.v[l]);
  g.h = sf_pose_out_size(g.v[SF_POSE_CONVS].H, 2, 2);
  g.w = sf_pose_out_size(g.v[SF_POSE_CONVS].W, 2, 2);
  SF_CHECK(g.h > 0 && g.w > 0, "%s: frames of %dx%d give no tokens", who, H, W);
  return 0;
}

struct StreamBufs { char *in, *a, *b, *rows; size_t bytes; };

// windows of 2 + cap frames: level 0 in `in`, odd levels in a, even levels in b (a level's window is dead once the next
// level's frames are computed and its last two frames are saved); rows: the gathered rows of the token embedding
int stream_carve(void* scratch, const StreamGeo& g, int n, StreamBufs& r, const char* who) {
  size_t sa = 0, sb = 0;
  for (int l = 0; l < SF_POSE_LEVELS; ++l) {
    const long b = (long)(2 + stream_cap(l, n)) * (long)g.frame[l];
    SF_CHECK(b < VOL_LIMIT, "%s: a window of %d frames of %dx%d with %d channels is %ld bytes, beyond the 4 GiB the convolution's 32-bit offsets cover; "
             "push fewer frames at a time", who, 2 + stream_cap(l, n), g.v[l].H, g.v[l].W, g.v[l].C, b);
    if (l == 0) continue;
    size_t& s = (l & 1) ? sa : sb;
    if ((size_t)b > s) s = (size_t)b;
  }
  Carve c(scratch);
  r.in = c.take((size_t)(2 + stream_cap(0, n)) * g.frame[0]);
  r.a = c.take(sa);
  r.b = c.take(sb);
  r.rows = c.take((size_t)stream_cap(SF_POSE_CONVS, n) * g.h * g.w * 64 * 2);
  r.bytes = c.off;
  return 0;
}

inline char* state_of(void* state, const StreamGeo& g, int l) {
  Carve c(state);
  char* r = nullptr;
  for (int i = 0; i <= l; ++i) r = c.take(2 * g.frame[i]);
  return r;
}

inline int copy2(char* dst, const char* src, size_t frame_bytes, void* stream) {
  return sf_hip_ok(hipMemcpyAsync(dst, src, 2 * frame_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "sf_pose_stream_push", "history copy");
}

}  // namespace

extern "C" int sf_pose_stream_plan(int frames_before, int n, int closing, sf_pose_push_plan* out) {
  const char* who = "sf_pose_stream_plan";
  SF_CHECK(out != nullptr, "%s: null plan", who);
  SF_CHECK(frames_before >= 0 && n >= 0 && frames_before <= STREAM_MAX_FRAMES && n <= STREAM_MAX_FRAMES, "%s: frames_before=%d n=%d", who, frames_before, n);
  SF_CHECK(!closing || frames_before + n > 0, "%s: closing a clip of no frames (frames_before=%d, n=%d)", who, frames_before, n);
  int f0[SF_POSE_LEVELS], f1[SF_POSE_LEVELS];
  stream_frontier(frames_before, false, f0);
  stream_frontier(frames_before + n, closing != 0, f1);
  for (int l = 0; l < SF_POSE_LEVELS; ++l) {
    out->first[l] = f0[l];
    out->count[l] = f1[l] - f0[l];
  }
  return 0;
}

extern "C" size_t sf_pose_stream_state_bytes(const sf_pose_model* model, int H, int W) {
  StreamGeo g;
  if (stream_geo(model, H, W, g, "sf_pose_stream_state_bytes") != 0) return 0;
  Carve c(nullptr);
  for (int l = 0; l < SF_POSE_CONVS; ++l) c.take(2 * g.frame[l]);
  return c.off;
}

extern "C" size_t sf_pose_stream_scratch_bytes(const sf_pose_model* model, int n_max, int H, int W) {
  const char* who = "sf_pose_stream_scratch_bytes";
  StreamGeo g;
  if (stream_geo(model, H, W, g, who) != 0) return 0;
  if (n_max < 0 || n_max > (1 << 20)) {
    sf_set_error("%s: n_max=%d", who, n_max);
    return 0;
  }
  StreamBufs b;
  if (stream_carve(nullptr, g, n_max, b, who) != 0) return 0;
  return b.bytes;
}

extern "C" int sf_pose_stream_push(const sf_pose_model* model, void* state, int frames_before, const void* frames, int dtype, int n, int H, int W,
                                   int closing, void* scratch, size_t scratch_bytes, void* tokens_out, int64_t token_rows_capacity,
                                   int32_t* latent_frames_written, void* stream) {
  const char* who = "sf_pose_stream_push";
  StreamGeo g;
  SF_TRY(stream_geo(model, H, W, g, who));
  SF_CHECK(state && scratch && latent_frames_written, "%s: null buffer", who);
  SF_CHECK(n >= 0 && n <= (1 << 20) && (n == 0 || frames != nullptr), "%s: n=%d frames%s", who, n, frames ? "" : " in a null buffer");
  SF_CHECK(dtype >= SF_POSE_U8 && dtype <= SF_POSE_BF16, "%s: unknown dtype %d", who, dtype);
  SF_CHECK((uintptr_t)state % 256 == 0 && (uintptr_t)scratch % 256 == 0, "%s: state and scratch must be 256-byte aligned", who);
  sf_pose_push_plan pl;
  SF_CHECK(sf_pose_stream_plan(frames_before, n, closing, &pl) == 0, "%s: frames_before=%d n=%d closing=%d: a clip of no frames cannot be closed, and counts are not negative",
           who, frames_before, n, closing);
  StreamBufs b;
  SF_TRY(stream_carve(scratch, g, n, b, who));
  SF_CHECK(scratch_bytes >= b.bytes, "%s: scratch of %zu bytes, %zu needed for a push of %d frames", who, scratch_bytes, b.bytes, n);
  for (int l = 0; l < SF_POSE_LEVELS; ++l)
    SF_CHECK(pl.count[l] >= 0 && pl.count[l] <= stream_cap(l, n), "%s: level %d gains %d frames, its window is planned for %d", who, l, pl.count[l],
             stream_cap(l, n));
  const int m = pl.count[SF_POSE_CONVS];
  const long rows = (long)m * g.h * g.w;
  SF_CHECK(token_rows_capacity >= rows, "%s: tokens_out holds %ld rows, this push writes %d x %d x %d = %ld", who, (long)token_rows_capacity, m, g.h, g.w, rows);
  SF_CHECK(m == 0 || (tokens_out && (uintptr_t)tokens_out % 16 == 0), "%s: tokens_out must be a 16-byte aligned buffer", who);
  *latent_frames_written = 0;
  if (n == 0 && !closing) return 0;

  char* win[SF_POSE_LEVELS];
  for (int l = 0; l < SF_POSE_LEVELS; ++l) win[l] = l == 0 ? b.in : (l & 1) ? b.a : b.b;
  // level 0: history, then the new frames prepared behind it
  if (frames_before > 0) SF_TRY(copy2(win[0], state_of(state, g, 0), g.frame[0], stream));
  if (n > 0) SF_TRY(sf_pose_prepare(frames, dtype, 0, n, H, W, frames_before == 0 ? 3 : 0, win[0] + 2 * g.frame[0], stream));
  if (!closing) SF_TRY(copy2(state_of(state, g, 0), win[0] + (size_t)pl.count[0] * g.frame[0], g.frame[0], stream));
  for (int i = 0; i < SF_POSE_CONVS; ++i) {
    const int l = i + 1;
    const bool keeps = l < SF_POSE_CONVS;      // the last level feeds the token embedding, not a convolution
    if (keeps && frames_before > 0) SF_TRY(copy2(win[l], state_of(state, g, l), g.frame[l], stream));
    if (pl.count[l] > 0) {
      const sf_pose_layer& L = model->conv[i];
      sf_pose_conv_args a;
      memset(&a, 0, sizeof(a));
      a.x = win[i]; a.w = L.w; a.bias = L.bias; a.out = win[l] + (keeps ? 2 * g.frame[l] : 0);
      a.T = 2 + pl.count[i]; a.H = g.v[i].H; a.W = g.v[i].W; a.Cin = L.cin; a.Cout = L.cout;
      a.kt = 3; a.stride_t = L.stride_t; a.stride_s = L.stride_s; a.ldw = L.ldw; a.ldo = 16; a.silu = L.silu;
      sf_pose_window w;
      w.x_t0 = pl.first[i] - 2; w.t_end = pl.first[i] + pl.count[i]; w.closed = closing ? 1 : 0;
      w.t_out0 = pl.first[l]; w.n_out = pl.count[l];
      SF_TRY(sf_pose_conv_window(&a, &w, stream));
    }
    if (keeps && !closing) SF_TRY(copy2(state_of(state, g, l), win[l] + (size_t)pl.count[l] * g.frame[l], g.frame[l], stream));
  }
  if (m > 0) {
    const Vol& v = g.v[SF_POSE_CONVS];
    SF_TRY(sf_pose_patch_embed(win[SF_POSE_CONVS], m, v.H, v.W, model->embed_w, model->embed_b, model->pose_dim, b.rows, tokens_out, stream));
  }
  *latent_frames_written = m;
  return 0;
}
