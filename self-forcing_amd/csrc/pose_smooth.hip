// Pose smoother (gfx950): a One-Euro filter on x and y of every keypoint, with a bounded hold across missing samples, on
// the device.  The definition of every number is self_forcing_amd/pose_smooth_reference.py (`frames`): float32, every
// sub, mul, add and div rounded on its own.  This file equals it bit for bit, so contraction is off for the whole file
// (csrc/pose_retarget.hip:1-7 says why a pragma and not intrinsics); `/` is correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt, and the kernel keeps subnormals.
//
// One launch per piece, one lane per (person, point): P * 134 lanes in workgroups of one wave.  A lane reads its 32 bytes
// of state as two 16-byte loads, walks the piece's n frames with the state in registers, and writes the state back as two
// 16-byte stores.  The filter is a dependent chain of three divisions per coordinate and frame; the sample of frame f + 1
// does not depend on it, so it is loaded before frame f's chain starts.  Every read lies inside src [n][P][134][3] and
// state [P][134][8]; every element of out [n][P][134][3] is written; the entry point refuses ranges that overlap.
#pragma clang fp contract(off)
#include <cmath>
#include "sf_frame_host.h"

namespace {

constexpr int THREADS = 64, STATE_BYTES = 32;
constexpr int MAX_GAP = 65535;
constexpr float TWO_PI = 0x1.921fb6p+2f;              // fp32(2 pi)

struct SmoothArgs {
  const float* src;                      // [n][P][134][3]
  float* out;                            // [n][P][134][3]
  uint4* state;                          // [P][134] x (hx, hy, dx, dy), (s, gap, seen, 0)
  int n, lanes;                          // lanes = P * 134
  float period, min_cutoff, beta, kd, threshold;
  int max_gap;
};

// pose_smooth_reference.frames, one coordinate: the new speed and position from the sample v
__device__ __forceinline__ void one_euro(float v, float te, float ad, float h, float d, float min_cutoff, float beta, float& hn, float& dn) {
  const float e = v - h;
  const float dx = e / te;
  float t = dx - d;
  t = ad * t;
  dn = d + t;
  float fc = beta * fabsf(dn);
  fc = min_cutoff + fc;
  float r = TWO_PI * fc;
  r = r * te;
  const float a = r / (r + 1.f);
  t = a * e;
  hn = h + t;
}

struct Filter {
  float hx, hy, dx, dy, s;
  int gap;
  bool seen;
};

struct Sample {
  float x, y, s;
};

__device__ __forceinline__ Sample load(const float* p) { return {p[0], p[1], p[2]}; }

__device__ __forceinline__ void store(float* o, Sample v) { o[0] = v.x, o[1] = v.y, o[2] = v.s; }

// one frame of one point: advances the state and returns the output
__device__ __forceinline__ Sample step(Filter& k, Sample in, const SmoothArgs& a) {
  const bool ok = isfinite(in.x) && isfinite(in.y) && isfinite(in.s) && in.s >= a.threshold && in.x >= 0.f && in.y >= 0.f;
  const float vx = ok ? in.x : 0.f, vy = ok ? in.y : 0.f;
  const float te = (float)(k.gap + 1) * a.period;
  const float rd = a.kd * te;
  const float ad = rd / (rd + 1.f);
  float hxn, hyn, dxn, dyn;
  one_euro(vx, te, ad, k.hx, k.dx, a.min_cutoff, a.beta, hxn, dxn);
  one_euro(vy, te, ad, k.hy, k.dy, a.min_cutoff, a.beta, hyn, dyn);
  const bool filt = ok && k.seen && isfinite(hxn) && isfinite(hyn) && isfinite(dxn) && isfinite(dyn);
  const bool hold = !ok && k.seen && k.gap < a.max_gap;
  if (ok) {
    k.hx = filt ? hxn : vx, k.hy = filt ? hyn : vy;
    k.dx = filt ? dxn : 0.f, k.dy = filt ? dyn : 0.f;
    k.s = in.s;
  }
  k.gap = hold ? k.gap + 1 : 0;
  k.seen = ok || hold;
  return {k.seen ? k.hx : ABSENT_XY, k.seen ? k.hy : ABSENT_XY, k.seen ? k.s : ABSENT_SCORE};
}

// Frame f + 1 is loaded before frame f's chain starts and frame f is stored behind it.  The first frame is peeled off the
// loop and the last iteration loads the last frame once more instead of a frame past the end, so the loop has one path
// and one shape of outstanding memory operations, and waits for frame f's sample alone.  (With the load under
// `if (f + 1 < n)` the two paths met in a wait for everything outstanding, the sample just asked for included; with the
// store in front of the load the compiler moved the load into the iteration that uses it.)
__global__ __launch_bounds__(THREADS) void pose_smooth_kernel(SmoothArgs a) {
  const int lane = blockIdx.x * THREADS + threadIdx.x;
  if (lane >= a.lanes) return;
  uint4* st = a.state + 2 * (size_t)lane;
  const uint4 w0 = st[0], w1 = st[1];
  Filter k = {__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z), __uint_as_float(w0.w), __uint_as_float(w1.x), (int)w1.y, w1.z != 0};

  const size_t stride = (size_t)a.lanes * 3;
  const float* __restrict__ p = a.src + (size_t)lane * 3;
  float* __restrict__ o = a.out + (size_t)lane * 3;
  Sample cur = load(p);
  Sample nxt = load(p + (a.n > 1 ? stride : 0));
  store(o, step(k, cur, a));                           // frame 0
  for (int f = 1; f < a.n; ++f) {
    cur = nxt;
    p += stride, o += stride;                          // frame f
    nxt = load(p + (f + 1 < a.n ? stride : 0));        // frame f + 1, in flight under frame f's chain
    store(o, step(k, cur, a));
  }
  st[0] = make_uint4(__float_as_uint(k.hx), __float_as_uint(k.hy), __float_as_uint(k.dx), __float_as_uint(k.dy));
  st[1] = make_uint4(__float_as_uint(k.s), (unsigned)k.gap, k.seen ? 1u : 0u, 0u);
}

}  // namespace

extern "C" size_t sf_pose_smooth_state_bytes(int people) {
  return people >= 1 && people <= SF_POSE_RENDER_MAX_PEOPLE ? (size_t)people * POINTS * STATE_BYTES : 0;
}

extern "C" int sf_pose_smooth_frames(const sf_pose_smooth_args* args, void* stream) {
  const char* who = "sf_pose_smooth_frames";
  SF_CHECK(args, "%s: null args", who);
  SF_CHECK(args->src && args->out && args->state, "%s: null buffer", who);
  SF_CHECK(args->people > 0 && args->people <= SF_POSE_RENDER_MAX_PEOPLE, "%s: people=%d (1..%d)", who, args->people, SF_POSE_RENDER_MAX_PEOPLE);
  SF_CHECK(args->n > 0 && args->n <= SF_POSE_RETARGET_MAX_FRAMES, "%s: n=%d (1..%d)", who, args->n, SF_POSE_RETARGET_MAX_FRAMES);
  SF_CHECK(args->max_gap >= 0 && args->max_gap <= MAX_GAP, "%s: max_gap=%d (0..%d)", who, args->max_gap, MAX_GAP);
  SF_CHECK((uintptr_t)args->src % 4 == 0 && (uintptr_t)args->out % 4 == 0, "%s: src and out must be 4-byte aligned", who);
  SF_CHECK((uintptr_t)args->state % 16 == 0, "%s: state must be 16-byte aligned", who);
  SF_CHECK(std::isfinite(args->period) && args->period > 0.f, "%s: period must be finite and > 0", who);
  SF_CHECK(std::isfinite(args->min_cutoff) && args->min_cutoff > 0.f, "%s: min_cutoff must be finite and > 0", who);
  SF_CHECK(std::isfinite(args->beta) && args->beta >= 0.f, "%s: beta must be finite and >= 0", who);
  SF_CHECK(std::isfinite(args->kd) && args->kd > 0.f, "%s: kd must be finite and > 0", who);
  SF_CHECK(std::isfinite(args->score_threshold), "%s: score_threshold must be finite", who);
  const int lanes = args->people * POINTS;
  const size_t frames_bytes = (size_t)args->n * lanes * 3 * sizeof(float), state_bytes = (size_t)lanes * STATE_BYTES;
  const Range range[3] = {{"src", args->src, frames_bytes}, {"out", args->out, frames_bytes}, {"state", args->state, state_bytes}};
  SF_TRY(disjoint(who, range));
  SmoothArgs a;
  a.src = args->src, a.out = args->out, a.state = (uint4*)args->state;
  a.n = args->n, a.lanes = lanes;
  a.period = args->period, a.min_cutoff = args->min_cutoff, a.beta = args->beta, a.kd = args->kd, a.threshold = args->score_threshold;
  a.max_gap = args->max_gap;
  return sf_launch<&pose_smooth_kernel>(who, dim3((unsigned)((lanes + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
}
