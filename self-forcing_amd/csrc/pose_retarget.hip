// Pose retargeter (gfx950): driving keypoints are lifted to output pixels, resampled to the generator's frame rate and
// given the reference person's proportions and position, on the device.  The definition of every number is
// self_forcing_amd/pose_retarget_reference.py (`lift`, `resample`, `fit`, `retarget_frame`): float32, every operation
// rounded on its own.  This file equals it bit for bit, so contraction is off for the whole file: hipcc would otherwise
// fuse a * b + c, and the __f*_rn intrinsics are plain operators here (a product inside one could still fuse with the add
// behind it; __fsqrt_rn is the native, 1-ulp square root).  `/` and sqrtf are correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt.
//
// One launch per piece, one workgroup of 192 threads per (output frame, person):
//   step 1  lanes 0..133 load their point of source frames i0 and i1, lift and resample it; lanes 134..151 and 152..169
//           lift the 18 body points of clip frame 0 (S0) and of the reference (R).  All of it goes to LDS.
//   step 2  lanes 0..16 measure their limb in S0 and R; lane 0 then adds the lengths in LIMBS order, forms g and the nine
//           group ratios, and walks the 17-step chain from the neck (each step reads what the step before wrote).
//   step 3  lanes 0..133 take their body point from the chain or place their attached point (feet, face, hands) from its
//           anchor, and store (x, y, score) or the (-1, -1, 0) marker.
// Every read lies inside src [n_src][P][134][3], first [P][134][3] and ref [ref_people][134][3] (the entry point checks
// that i0 and i1 of every requested frame fall in the piece); every write inside out [n_out][P][134][3].
#pragma clang fp contract(off)
#include <cmath>
#include "sf_frame_host.h"

namespace {

constexpr int EDGES = 17, GROUPS = 9, NECK = 1, THREADS = 192;
constexpr int HAND_GROUP = 2, FACE_GROUP = 7;         // the forearms {3, 5}, nose-eye {13, 15}
constexpr long MAX_INDEX = 1L << 40;                  // frame indices: index * 65535 stays far inside int64

__constant__ const uint8_t LIMB_A[EDGES] = {1, 1, 2, 3, 5, 6, 1, 8, 9, 1, 11, 12, 1, 0, 14, 0, 15};
__constant__ const uint8_t LIMB_B[EDGES] = {2, 5, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 0, 14, 16, 15, 17};
__constant__ const uint8_t GROUP_OF[EDGES] = {0, 0, 1, 2, 1, 2, 3, 4, 5, 3, 4, 5, 6, 7, 8, 7, 8};
__constant__ const int8_t GROUP_M0[GROUPS] = {0, 2, 3, 6, 7, 8, 12, 13, 14};
__constant__ const int8_t GROUP_M1[GROUPS] = {1, 4, 5, 9, 10, 11, -1, 15, 16};

struct RetargetArgs {
  const float* src;                      // [n_src][P][134][3], clip frames src0 ..
  const float* first;                    // [P][134][3], clip frame 0
  const float* ref;                      // [ref_people][134][3]
  float* out;                            // [n_out][P][134][3], output frames out0 ..
  long src0, out0;
  int P, ref_people, num, den;
  float ssx, ssy, rsx, rsy, threshold;
  int align;
};

struct Pt {
  float x, y, s;
  bool ok;
};

// pose_retarget_reference.lift: validity on the raw values, one multiply per coordinate
__device__ __forceinline__ Pt lift(const float* p, float sx, float sy, float threshold) {
  const float x = p[0], y = p[1], s = p[2];
  Pt r;
  r.ok = isfinite(x) && isfinite(y) && isfinite(s) && s >= threshold && x >= 0.f && y >= 0.f;
  r.x = r.ok ? x * sx : 0.f, r.y = r.ok ? y * sy : 0.f, r.s = r.ok ? s : 0.f;
  return r;
}

__device__ __forceinline__ float mix(float a, float b, float w) {
  float t = b - a;
  t = w * t;
  return a + t;
}

__device__ __forceinline__ float edge_length(const float* x, const float* y, int a, int b) {
  const float dx = x[b] - x[a], dy = y[b] - y[a];
  const float xx = dx * dx, yy = dy * dy;
  return sqrtf(xx + yy);
}

// base + r * (q - from), three roundings: a chain step, and sim() with (R[1], g, S0[1])
__device__ __forceinline__ float place(float base, float r, float q, float from) {
  float t = q - from;
  t = r * t;
  return base + t;
}

__global__ __launch_bounds__(THREADS) void pose_retarget_kernel(RetargetArgs a) {
  __shared__ float qx[POINTS], qy[POINTS];
  __shared__ int qok[POINTS];
  __shared__ float s0x[BODY], s0y[BODY], rx[BODY], ry[BODY], nx[BODY], ny[BODY];
  __shared__ int s0ok[BODY], rok[BODY], eok[EDGES];
  __shared__ float els[EDGES], elr[EDGES], ratio[GROUPS];
  __shared__ float s_g;

  const int t = threadIdx.x, person = blockIdx.y;
  const long pos = (a.out0 + blockIdx.x) * a.num, i0 = pos / a.den;
  const int rem = (int)(pos - i0 * a.den);
  Pt q = {0.f, 0.f, 0.f, false};
  if (t < POINTS) {
    const float* pa = a.src + (((i0 - a.src0) * a.P + person) * POINTS + t) * 3;
    const Pt A = lift(pa, a.ssx, a.ssy, a.threshold);
    q = A;
    if (rem != 0) {
      const Pt B = lift(pa + (long)a.P * POINTS * 3, a.ssx, a.ssy, a.threshold);
      const float w = (float)rem / (float)a.den;
      if (A.ok && B.ok) {
        q.x = mix(A.x, B.x, w), q.y = mix(A.y, B.y, w), q.s = B.s < A.s ? B.s : A.s;
      } else if (A.ok != B.ok) {
        const bool nearer_a = 2 * rem <= a.den;
        q = A.ok ? A : B;
        q.ok = A.ok == nearer_a;
      }
    }
    qx[t] = q.x, qy[t] = q.y, qok[t] = q.ok;
  } else if (t < POINTS + BODY) {
    const int k = t - POINTS;
    const Pt s = lift(a.first + ((long)person * POINTS + k) * 3, a.ssx, a.ssy, a.threshold);
    s0x[k] = s.x, s0y[k] = s.y, s0ok[k] = s.ok;
  } else if (t < POINTS + 2 * BODY) {
    const int k = t - POINTS - BODY;
    const Pt r = lift(a.ref + ((long)(a.ref_people == 1 ? 0 : person) * POINTS + k) * 3, a.rsx, a.rsy, a.threshold);
    rx[k] = r.x, ry[k] = r.y, rok[k] = r.ok;
  }
  float ox = q.x, oy = q.y;
  if (a.align) {                                       // uniform: every lane takes the same way to each barrier
    __syncthreads();
    if (s0ok[NECK] && rok[NECK]) {                     // uniform; no anchor, no retarget
      if (t < EDGES) {
        const int ea = LIMB_A[t], eb = LIMB_B[t];
        bool ok = s0ok[ea] && s0ok[eb] && rok[ea] && rok[eb];
        const float ls = ok ? edge_length(s0x, s0y, ea, eb) : 0.f;
        ok = ok && ls > 0.f;
        els[t] = ls, elr[t] = ok ? edge_length(rx, ry, ea, eb) : 0.f, eok[t] = ok;
      }
      __syncthreads();
      if (t == 0) {
        float sum_r = 0.f, sum_s = 0.f;
        bool any = false;
        for (int e = 0; e < EDGES; ++e)
          if (eok[e]) sum_r = sum_r + elr[e], sum_s = sum_s + els[e], any = true;
        const float g = any ? sum_r / sum_s : 1.f;
        s_g = g;
        for (int k = 0; k < GROUPS; ++k) {
          const int m0 = GROUP_M0[k], m1 = GROUP_M1[k];
          const bool u0 = eok[m0], u1 = m1 >= 0 && eok[m1];
          const float r0 = u0 ? elr[m0] / els[m0] : 0.f, r1 = u1 ? elr[m1] / els[m1] : 0.f;
          ratio[k] = u0 && u1 ? (r0 + r1) * 0.5f : (u0 ? r0 : (u1 ? r1 : g));
        }
        nx[NECK] = place(rx[NECK], g, qx[NECK], s0x[NECK]), ny[NECK] = place(ry[NECK], g, qy[NECK], s0y[NECK]);
        for (int e = 0; e < EDGES; ++e) {
          const int ea = LIMB_A[e], eb = LIMB_B[e];
          if (!qok[eb]) continue;
          if (qok[ea]) {
            const float r = ratio[GROUP_OF[e]];
            nx[eb] = place(nx[ea], r, qx[eb], qx[ea]), ny[eb] = place(ny[ea], r, qy[eb], qy[ea]);
          } else {
            nx[eb] = place(rx[NECK], g, qx[eb], s0x[NECK]), ny[eb] = place(ry[NECK], g, qy[eb], s0y[NECK]);
          }
        }
      }
      __syncthreads();
      if (t < BODY) {
        ox = nx[t], oy = ny[t];
      } else if (t < POINTS && q.ok) {
        const int anchor = t < 21 ? 13 : (t < 24 ? 10 : (t < 92 ? 0 : (t < 113 ? 7 : 4)));
        const float g = s_g, r = t < 24 ? g : (t < 92 ? ratio[FACE_GROUP] : ratio[HAND_GROUP]);
        if (qok[anchor])
          ox = place(nx[anchor], r, q.x, qx[anchor]), oy = place(ny[anchor], r, q.y, qy[anchor]);
        else
          ox = place(rx[NECK], g, q.x, s0x[NECK]), oy = place(ry[NECK], g, q.y, s0y[NECK]);
      }
    }
  }
  if (t < POINTS) {
    float* o = a.out + (((long)blockIdx.x * a.P + person) * POINTS + t) * 3;
    o[0] = q.ok ? ox : ABSENT_XY, o[1] = q.ok ? oy : ABSENT_XY, o[2] = q.ok ? q.s : ABSENT_SCORE;
  }
}

// the output frames a clip of `frames` source frames gives (pose_retarget_reference.frames_out)
inline long frames_out(long frames, long num, long den) { return frames <= 0 ? 0 : ((frames - 1) * den) / num + 1; }

}  // namespace

extern "C" int sf_pose_retarget_plan(int64_t frames_before, int64_t n, int num, int den, int64_t* first_out, int64_t* n_out) {
  const char* who = "sf_pose_retarget_plan";
  SF_CHECK(first_out && n_out, "%s: null result", who);
  SF_CHECK(frames_before >= 0 && n >= 0 && frames_before <= MAX_INDEX && n <= MAX_INDEX, "%s: frames_before=%ld n=%ld (0..2^40)", who,
           (long)frames_before, (long)n);
  SF_CHECK(num >= 1 && num <= SF_POSE_RETARGET_MAX_RATE && den >= 1 && den <= SF_POSE_RETARGET_MAX_RATE, "%s: rate %d/%d (both 1..%d)", who, num, den,
           SF_POSE_RETARGET_MAX_RATE);
  *first_out = frames_out(frames_before, num, den);
  *n_out = frames_out(frames_before + n, num, den) - *first_out;
  return 0;
}

extern "C" int sf_pose_retarget_frames(const sf_pose_retarget_args* args, void* stream) {
  const char* who = "sf_pose_retarget_frames";
  SF_CHECK(args, "%s: null args", who);
  SF_CHECK(args->src && args->first && args->ref && args->out, "%s: null buffer", who);
  SF_CHECK(args->people > 0 && args->people <= SF_POSE_RENDER_MAX_PEOPLE, "%s: people=%d (1..%d)", who, args->people, SF_POSE_RENDER_MAX_PEOPLE);
  SF_CHECK(args->ref_people == 1 || args->ref_people == args->people, "%s: ref_people=%d (1 or people=%d)", who, args->ref_people, args->people);
  SF_CHECK(args->num >= 1 && args->num <= SF_POSE_RETARGET_MAX_RATE && args->den >= 1 && args->den <= SF_POSE_RETARGET_MAX_RATE,
           "%s: rate %d/%d (both 1..%d)", who, args->num, args->den, SF_POSE_RETARGET_MAX_RATE);
  SF_CHECK(args->n_src > 0 && args->n_out > 0 && args->n_out <= SF_POSE_RETARGET_MAX_FRAMES, "%s: n_src=%d, n_out=%d (n_src >= 1, n_out 1..%d)", who,
           args->n_src, args->n_out, SF_POSE_RETARGET_MAX_FRAMES);
  SF_CHECK(args->src0 >= 0 && args->out0 >= 0 && args->src0 <= MAX_INDEX && args->out0 <= MAX_INDEX, "%s: src0=%ld out0=%ld (0..2^40)", who,
           (long)args->src0, (long)args->out0);
  SF_CHECK(std::isfinite(args->src_sx) && std::isfinite(args->src_sy) && std::isfinite(args->ref_sx) && std::isfinite(args->ref_sy),
           "%s: scale factors must be finite", who);
  SF_CHECK(std::isfinite(args->score_threshold), "%s: score_threshold must be finite", who);
  SF_CHECK(args->align == 0 || args->align == 1, "%s: align=%d (0 or 1)", who, args->align);
  SF_CHECK((uintptr_t)args->src % 4 == 0 && (uintptr_t)args->first % 4 == 0 && (uintptr_t)args->ref % 4 == 0 && (uintptr_t)args->out % 4 == 0,
           "%s: buffers must be 4-byte aligned", who);
  // the source frames the outputs read: i0 of the first, i1 = ceil(j num / den) of the last
  const long j_last = args->out0 + args->n_out - 1;
  const long i_lo = args->out0 * args->num / args->den, i_hi = (j_last * args->num + args->den - 1) / args->den;
  SF_CHECK(i_lo >= args->src0 && i_hi <= args->src0 + args->n_src - 1, "%s: output frames [%ld, %ld] read source frames [%ld, %ld], the piece holds [%ld, %ld]",
           who, (long)args->out0, j_last, i_lo, i_hi, (long)args->src0, (long)args->src0 + args->n_src - 1);
  RetargetArgs a;
  a.src = args->src, a.first = args->first, a.ref = args->ref, a.out = args->out;
  a.src0 = args->src0, a.out0 = args->out0;
  a.P = args->people, a.ref_people = args->ref_people, a.num = args->num, a.den = args->den;
  a.ssx = args->src_sx, a.ssy = args->src_sy, a.rsx = args->ref_sx, a.rsy = args->ref_sy, a.threshold = args->score_threshold;
  a.align = args->align;
  return sf_launch<&pose_retarget_kernel>(who, dim3((unsigned)args->n_out, (unsigned)args->people), dim3(THREADS), 0, (hipStream_t)stream, a);
}
