// Pose tracker (gfx950): the people a detector lists per frame, in any order -> each person in one stable slot across
// frames, on the device.  The definition of every number is self_forcing_amd/pose_track_reference.py (`frames`): float32,
// every sub, mul, add and div rounded on its own.  This file equals it bit for bit, so contraction is off for the whole
// file (csrc/pose_retarget.hip:1-7 says why a pragma and not intrinsics); `/` is correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt, and the kernels keep subnormals.
//
// Two kernels behind one C call, on one stream.  The ASSIGNMENT kernel is serial in frames and tiny per frame: one wave,
// lane = 8 * slot + detection.  The packed state [S + 1][40] is read once into LDS and written once from it.  A lane holds
// the x, y and validity of its detection's 18 body points in registers (the 54 floats of frame f + 1 are loaded before
// frame f's chain starts), reads its slot's memory from LDS, runs the 18-point cost chain in the definition's order, and
// the greedy rounds are wave-wide minima of a 64-bit key (cost bits : lane) by DPP, with no LDS round trip.  Age and birth
// run on every lane of a slot's row alike; the lane (slot, its detection) replaces the slot's memory in LDS.  Per frame it
// writes assign[f][s] (the detection index or -1) and ids[f][s].  The GATHER kernel is parallel over (frame, slot, element):
// it copies src[f][assign[f][s]] or writes the marker into all n * S * 402 floats of out.
// Every read lies inside src [n][P][134][3], state [S + 1][40] and assign [n][S] (a detection index outside 0..P-1 cannot
// come out of the assignment kernel, and the gather kernel writes the marker for one anyway); every element of out, ids and
// assign is written; the entry point refuses ranges that overlap.
#pragma clang fp contract(off)
#include <cmath>
#include "sf_frame_host.h"

namespace {

constexpr int ROW = POINTS * 3, WAVE = 64, GRID = 8;
constexpr int STATE_WORDS = 40, W_MASK = 36, W_AGE = 37, W_ID = 38, W_ALIVE = 39;
constexpr int MAX_AGE = 65535, GATHER_THREADS = 256;

struct TrackArgs {
  const float* src;                      // [n][P][134][3]
  int* assign;                           // [n][S]
  int* ids;                              // [n][S]
  uint4* state;                          // [S + 1][10]
  int n, people, slots;
  int min_points, min_common, max_age;
  float gate2, threshold;
};

struct GatherArgs {
  const float* src;                      // [n][P][134][3]
  const int* assign;                     // [n][S]
  float* out;                            // [n][S][134][3]
  size_t total;                          // n * S * 402
  int people, slots;
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xF, false);
}

// one step of the wave-wide minimum of (hi, lo) as one unsigned 64-bit number; lanes the row mask leaves out read themselves
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void min_step(unsigned& hi, unsigned& lo) {
  const unsigned ohi = dpp<CTRL, ROW_MASK>(hi), olo = dpp<CTRL, ROW_MASK>(lo);
  const bool less = ohi < hi || (ohi == hi && olo < lo);
  hi = less ? ohi : hi, lo = less ? olo : lo;
}

// the smallest key of the wave, in every lane (sf_common.h's wave_max says what the six controls do); all 64 lanes active
__device__ __forceinline__ void wave_min_key(unsigned& hi, unsigned& lo) {
  min_step<0xB1, 0xF>(hi, lo);
  min_step<0x4E, 0xF>(hi, lo);
  min_step<0x141, 0xF>(hi, lo);
  min_step<0x140, 0xF>(hi, lo);
  min_step<0x142, 0xA>(hi, lo);
  min_step<0x143, 0xC>(hi, lo);
  hi = (unsigned)__builtin_amdgcn_readlane((int)hi, 63), lo = (unsigned)__builtin_amdgcn_readlane((int)lo, 63);
}

// bit t of the result = bit 8 t of the ballot: the lanes (t, 0)
__device__ __forceinline__ unsigned rows_of(unsigned long long ballot) {
  return (unsigned)(((ballot & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
}

struct Detection {
  float x[BODY], y[BODY];
  unsigned ok;                           // bit j: point j is valid
};

struct Raw {
  float v[BODY * 3];
};

__device__ __forceinline__ Raw load(const float* p) {
  Raw r;
#pragma unroll
  for (int i = 0; i < BODY * 3; ++i) r.v[i] = p[i];
  return r;
}

__device__ __forceinline__ Detection judge(const Raw& r, float threshold) {
  Detection d;
  d.ok = 0;
#pragma unroll
  for (int j = 0; j < BODY; ++j) {
    const float x = r.v[3 * j], y = r.v[3 * j + 1], s = r.v[3 * j + 2];
    d.x[j] = x, d.y[j] = y;
    d.ok |= (isfinite(x) && isfinite(y) && isfinite(s) && s >= threshold && x >= 0.f && y >= 0.f) ? 1u << j : 0u;
  }
  return d;
}

struct Row {                             // a slot, the same in the 8 lanes of its row
  int age, id;
  bool alive;
};

// one frame: matches, ages and births; returns the detection of this lane's slot or -1
__device__ __forceinline__ int step(const TrackArgs& a, const int* mem, int lane, const Detection& det, Row& row, unsigned& next_id, int* st) {
  const int t = lane >> 3, d = lane & 7;
  const bool active = t < a.slots && d < a.people;
  // pose_track_reference.costs: the chain over the points valid in both, and the extents of the slot's valid points
  const unsigned tm = (unsigned)mem[W_MASK], common = tm & det.ok;
  float acc = 0.f, max_x = -INFINITY, min_x = INFINITY, max_y = -INFINITY, min_y = INFINITY;
#pragma unroll
  for (int j = 0; j < BODY; ++j) {
    const float xt = __int_as_float(mem[2 * j]), yt = __int_as_float(mem[2 * j + 1]);
    const float dx = det.x[j] - xt, dy = det.y[j] - yt;
    float q = dx * dx;
    const float qy = dy * dy;
    q = q + qy;
    const float sum = acc + q;
    acc = (common >> j & 1u) ? sum : acc;
    const bool in = tm >> j & 1u;
    max_x = in && xt > max_x ? xt : max_x, min_x = in && xt < min_x ? xt : min_x;
    max_y = in && yt > max_y ? yt : max_y, min_y = in && yt < min_y ? yt : min_y;
  }
  const int n = __popc(common);
  const float w = max_x - min_x, h = max_y - min_y;
  const float ww = w * w, hh = h * h;
  const float s2 = ww + hh;
  float cost = acc / (float)n;
  cost = cost / s2;
  const bool person = d < a.people && __popc(det.ok) >= a.min_points;
  const bool admissible = active && row.alive && person && n >= a.min_common && s2 > 0.f && isfinite(s2) && isfinite(cost) && cost <= a.gate2;
  unsigned hi = admissible ? __float_as_uint(cost) : 0xFFFFFFFFu, lo = admissible ? (unsigned)lane : 0xFFFFFFFFu;

  const unsigned persons = (unsigned)__ballot(person && t == 0) & 0xFFu;
  const unsigned free0 = ~rows_of(__ballot(row.alive && d == 0)) & ((1u << a.slots) - 1u);     // free at the start of this frame
  // 1 match: at most min(S, P) rounds, each a wave-wide minimum
  int mine = -1;
  unsigned taken = 0;
  for (int r = 0; r < GRID; ++r) {
    unsigned mhi = hi, mlo = lo;
    wave_min_key(mhi, mlo);
    if (mhi == 0xFFFFFFFFu) break;
    const int wt = (int)(mlo >> 3), wd = (int)(mlo & 7u);
    mine = t == wt ? wd : mine;
    taken |= 1u << wd;
    if (t == wt || d == wd) hi = 0xFFFFFFFFu, lo = 0xFFFFFFFFu;
  }
  // 2 age
  if (row.alive) {
    row.age = mine >= 0 ? 0 : row.age + 1;
    row.alive = mine >= 0 || row.age <= a.max_age;
  }
  // 3 birth: the k-th free slot takes the k-th unassigned person
  unsigned waiting = persons & ~taken;
  const int born = min(__popc(free0), __popc(waiting));
  const int k = __popc(free0 & ((1u << t) - 1u));
  if ((free0 >> t & 1u) && k < born) {
#pragma unroll
    for (int i = 0; i < GRID - 1; ++i) waiting = i < k ? waiting & (waiting - 1u) : waiting;
    mine = __ffs(waiting) - 1;
    row.id = (int)((next_id + (unsigned)k) & 0x7FFFFFFFu);
    row.age = 0, row.alive = true;
  }
  next_id += (unsigned)born;
  // 4 the memory of a slot that has a detection is replaced, by the lane that holds that detection
  __syncthreads();                                      // every lane has read the old memory
  if (t < a.slots && mine == d) {
    int* m = st + t * STATE_WORDS;
#pragma unroll
    for (int j = 0; j < BODY; ++j) m[2 * j] = __float_as_int(det.x[j]), m[2 * j + 1] = __float_as_int(det.y[j]);
    m[W_MASK] = (int)det.ok;
  }
  __syncthreads();
  return mine;
}

// Frame f + 1's body points are loaded before frame f's chain starts, as in pose_smooth_kernel: the first frame is peeled
// off the loop and the last iteration loads the last frame once more instead of a frame past the end.
__global__ __launch_bounds__(WAVE) void pose_track_assign_kernel(TrackArgs a) {
  __shared__ __attribute__((aligned(16))) int st[(GRID + 1) * STATE_WORDS];
  const int lane = threadIdx.x, t = lane >> 3, d = lane & 7;
  const int words4 = (a.slots + 1) * (STATE_WORDS / 4);
  for (int i = lane; i < words4; i += WAVE) ((uint4*)st)[i] = a.state[i];
  __syncthreads();
  const int* mem = st + (t < a.slots ? t : 0) * STATE_WORDS;
  Row row = {mem[W_AGE], mem[W_ID], t < a.slots && mem[W_ALIVE] != 0};
  unsigned next_id = (unsigned)st[a.slots * STATE_WORDS];

  const size_t stride = (size_t)a.people * ROW;
  const float* __restrict__ p = a.src + (size_t)(d < a.people ? d : 0) * ROW;
  int* __restrict__ assign = a.assign;
  int* __restrict__ ids = a.ids;
  Raw nxt = load(p);
  for (int f = 0; f < a.n; ++f) {
    const Detection cur = judge(nxt, a.threshold);
    nxt = load(p + (f + 1 < a.n ? stride : 0));         // frame f + 1, in flight under frame f's chain
    p += f + 1 < a.n ? stride : 0;
    const int mine = step(a, mem, lane, cur, row, next_id, st);
    if (d == 0 && t < a.slots) {
      assign[(size_t)f * a.slots + t] = mine;
      ids[(size_t)f * a.slots + t] = mine >= 0 ? row.id : -1;
    }
  }
  if (d == 0 && t < a.slots) {
    int* m = st + t * STATE_WORDS;
    m[W_AGE] = row.age, m[W_ID] = row.id, m[W_ALIVE] = row.alive ? 1 : 0;
  }
  if (lane == 0) st[a.slots * STATE_WORDS] = (int)next_id;
  __syncthreads();
  for (int i = lane; i < words4; i += WAVE) a.state[i] = ((const uint4*)st)[i];
}

__global__ __launch_bounds__(GATHER_THREADS) void pose_track_gather_kernel(GatherArgs a) {
  const size_t i = (size_t)blockIdx.x * GATHER_THREADS + threadIdx.x;
  if (i >= a.total) return;
  const size_t row = i / ROW;                           // f * S + s
  const int e = (int)(i - row * ROW);
  const int d = a.assign[row];
  const size_t f = row / (size_t)a.slots;
  const float marker = e % 3 == 2 ? ABSENT_SCORE : ABSENT_XY;
  a.out[i] = d >= 0 && d < a.people ? a.src[(f * a.people + d) * ROW + e] : marker;
}

}  // namespace

extern "C" size_t sf_pose_track_state_bytes(int slots) {
  return slots >= 1 && slots <= SF_POSE_RENDER_MAX_PEOPLE ? (size_t)(slots + 1) * STATE_WORDS * 4 : 0;
}

extern "C" int sf_pose_track_frames(const sf_pose_track_args* args, void* stream) {
  const char* who = "sf_pose_track_frames";
  SF_CHECK(args, "%s: null args", who);
  SF_CHECK(args->src && args->out && args->ids && args->state && args->assign, "%s: null buffer", who);
  SF_CHECK(args->people > 0 && args->people <= SF_POSE_RENDER_MAX_PEOPLE, "%s: people=%d (1..%d)", who, args->people, SF_POSE_RENDER_MAX_PEOPLE);
  SF_CHECK(args->slots > 0 && args->slots <= SF_POSE_RENDER_MAX_PEOPLE, "%s: slots=%d (1..%d)", who, args->slots, SF_POSE_RENDER_MAX_PEOPLE);
  SF_CHECK(args->n > 0 && args->n <= SF_POSE_RETARGET_MAX_FRAMES, "%s: n=%d (1..%d)", who, args->n, SF_POSE_RETARGET_MAX_FRAMES);
  SF_CHECK(args->min_points >= 1 && args->min_points <= BODY, "%s: min_points=%d (1..%d)", who, args->min_points, BODY);
  SF_CHECK(args->min_common >= 1 && args->min_common <= BODY, "%s: min_common=%d (1..%d)", who, args->min_common, BODY);
  SF_CHECK(args->max_age >= 0 && args->max_age <= MAX_AGE, "%s: max_age=%d (0..%d)", who, args->max_age, MAX_AGE);
  SF_CHECK((uintptr_t)args->src % 4 == 0 && (uintptr_t)args->out % 4 == 0, "%s: src and out must be 4-byte aligned", who);
  SF_CHECK((uintptr_t)args->ids % 4 == 0 && (uintptr_t)args->assign % 4 == 0, "%s: ids and assign must be 4-byte aligned", who);
  SF_CHECK((uintptr_t)args->state % 16 == 0, "%s: state must be 16-byte aligned", who);
  SF_CHECK(std::isfinite(args->gate2) && args->gate2 > 0.f, "%s: gate2 must be finite and > 0", who);
  SF_CHECK(std::isfinite(args->score_threshold), "%s: score_threshold must be finite", who);
  const size_t rows = (size_t)args->n * args->slots;
  const Range range[5] = {{"src", args->src, (size_t)args->n * args->people * ROW * sizeof(float)},
                          {"out", args->out, rows * ROW * sizeof(float)},
                          {"ids", args->ids, rows * sizeof(int32_t)},
                          {"state", args->state, sf_pose_track_state_bytes(args->slots)},
                          {"assign", args->assign, rows * sizeof(int32_t)}};
  SF_TRY(disjoint(who, range));
  TrackArgs a;
  a.src = args->src, a.assign = args->assign, a.ids = args->ids, a.state = (uint4*)args->state;
  a.n = args->n, a.people = args->people, a.slots = args->slots;
  a.min_points = args->min_points, a.min_common = args->min_common, a.max_age = args->max_age;
  a.gate2 = args->gate2, a.threshold = args->score_threshold;
  SF_TRY(sf_launch<&pose_track_assign_kernel>(who, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, a));
  GatherArgs g;
  g.src = args->src, g.assign = args->assign, g.out = args->out;
  g.total = rows * ROW, g.people = args->people, g.slots = args->slots;
  return sf_launch<&pose_track_gather_kernel>(who, dim3((unsigned)((g.total + GATHER_THREADS - 1) / GATHER_THREADS)), dim3(GATHER_THREADS), 0,
                                              (hipStream_t)stream, g);
}
