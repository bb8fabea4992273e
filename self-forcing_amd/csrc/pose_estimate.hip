// The DWPose glue (gfx950): what DWPose does around its two networks in numpy and OpenCV on the host, on the device.
// YOLOX head -> person boxes (decode + greedy NMS), boxes -> the pose network's input crops, SimCC logits -> whole-body
// keypoints in the renderer's layout.  The definition of every number is self_forcing_amd/pose_estimate_reference.py:
// float32, every add, sub, mul and div rounded on its own.  This file equals it bit for bit, so contraction is off for the
// whole file (csrc/pose_retarget.hip:1-7 says why a pragma and not intrinsics); `/` is correctly rounded under hipcc's
// default -fhip-fp32-correctly-rounded-divide-sqrt, rintf / floorf / ldexpf are exact, and the kernels keep subnormals.
//
// Four kernels behind three C calls.
//   boxes   A wide CANDIDATE kernel (a lane per (frame, anchor)) writes the live score (0 = no candidate) and the four
//           source-frame corners to caller-owned scratch [F][5][A], so the exp32 and the divisions run once per anchor on
//           the whole device.  The NMS kernel is one workgroup of 1024 lanes per frame: a lane keeps one live bit for each
//           of its <= 16 anchors, a round is a workgroup arg-max of the 64-bit key (score bits : ~anchor) by
//           shuffles and 16 words of LDS, then a sweep in which every lane that still holds a live anchor reads its
//           corners from scratch and compares.  Scratch was chosen over recomputing: the sweeps then read 16 bytes per
//           live anchor instead of redoing two exp32 and four divisions per anchor per round.
//   crops   a lane per four output pixels of a row (one where a row is no whole number of quads) and their three
//           channels; four taps per pixel and channel, zero outside the frame; 16-byte stores.
//   simcc   a workgroup of 16 waves per person; the waves share the 266 rows (133 points x 2 axes), 16-byte loads where
//           the rows are aligned, every lane's scan of four of a wave's 17 rows before their four shuffle arg-maxes on (value,
//           index) with the first index winning ties, results in LDS; after a barrier 134 lanes apply the neck, the reorder and the map back to the frame.
// Every read lies inside the tensors the entry points describe (an index is clamped where a load runs ahead of its
// bound), every element of every output is written, and the entry points refuse ranges that overlap.
#pragma clang fp contract(off)
#include <cmath>
#include "sf_frame_host.h"

namespace {

constexpr int WAVE = 64, SIMCC = SF_POSE_SIMCC_POINTS;
constexpr int CAND_THREADS = 256, CROP_THREADS = 256;
constexpr int NMS_THREADS = 1024, NMS_WAVES = NMS_THREADS / WAVE, NMS_PER = SF_POSE_BOXES_MAX_ANCHORS / NMS_THREADS;
constexpr int SIMCC_THREADS = 1024, SIMCC_WAVES = SIMCC_THREADS / WAVE, SIMCC_BATCH = 4;
constexpr int SIMCC_ROWS = (2 * SIMCC + SIMCC_WAVES - 1) / SIMCC_WAVES, SIMCC_GROUP = 4;       // rows per wave: 17, scanned 4 at a time

// ------------------------------------------------------------------------------------------ exp32 (pose_estimate_reference.exp32)
__device__ __forceinline__ float exp32(float x) {
  x = x < -20.0f ? -20.0f : (x > 20.0f ? 20.0f : x);                   // selects: NaN passes
  const float n = rintf(x * 1.4426950408889634f);
  float r = x - n * 0.693145751953125f;
  r = r - n * 1.428606765330187e-06f;
  float p = (float)(1.0 / 720.0);
  p = p * r, p = p + (float)(1.0 / 120.0);
  p = p * r, p = p + (float)(1.0 / 24.0);
  p = p * r, p = p + (float)(1.0 / 6.0);
  p = p * r, p = p + 0.5f;
  p = p * r, p = p + 1.0f;
  p = p * r, p = p + 1.0f;
  return ldexpf(p, n == n ? (int)n : 0);
}

// ------------------------------------------------------------------------------------------ the window of a box
struct Window {
  float cx, cy, ax, ay;
  bool valid;
};

// pose_estimate_reference.person_window: host and device share it, the crop and its inverse too
__host__ __device__ inline Window person_window(float x1, float y1, float x2, float y2, int out_h, int out_w, float padding) {
  Window w;
  w.cx = (x1 + x2) * 0.5f, w.cy = (y1 + y2) * 0.5f;
  float bw = (x2 - x1) * padding, bh = (y2 - y1) * padding;
  const float aspect = (float)out_w / (float)out_h;
  const float tall = bh * aspect;
  if (bw > tall) bh = bw / aspect;
  else bw = tall;
  w.ax = bw / (float)out_w, w.ay = bh / (float)out_h;
  w.valid = std::isfinite(w.cx) && std::isfinite(w.cy) && std::isfinite(bw) && std::isfinite(bh) && std::isfinite(w.ax) && std::isfinite(w.ay) &&
            bw > 0.f && bh > 0.f;
  return w;
}

// the window of person (f, p), valid only where p < count[f]
__device__ __forceinline__ Window window_of(const float* boxes, const int* count, int n, int people, int out_h, int out_w, float padding) {
  const float* b = boxes + (size_t)n * 5;
  Window w = person_window(b[0], b[1], b[2], b[3], out_h, out_w, padding);
  w.valid = w.valid && n % people < count[n / people];
  return w;
}

// ------------------------------------------------------------------------------------------ 1 boxes
struct CandArgs {
  const float* head;                     // [F][A][5 + C]
  float* scratch;                        // [F][5][A]: live score, x1, y1, x2, y2
  int A, row, cls;                       // row = 5 + C, cls = 5 + class_index
  int in_w, n_strides, strides[SF_POSE_BOXES_MAX_STRIDES], first[SF_POSE_BOXES_MAX_STRIDES];   // first anchor of each level
  int decoded;
  float ratio, threshold;
};

__global__ __launch_bounds__(CAND_THREADS) void pose_boxes_candidates_kernel(CandArgs a) {
  const int i = blockIdx.x * CAND_THREADS + threadIdx.x, f = blockIdx.y;
  if (i >= a.A) return;
  const float* __restrict__ o = a.head + ((size_t)f * a.A + i) * a.row;
  float cx = o[0], cy = o[1], w = o[2], h = o[3];
  if (!a.decoded) {
    int level = 0;
#pragma unroll
    for (int l = 1; l < SF_POSE_BOXES_MAX_STRIDES; ++l) level = l < a.n_strides && i >= a.first[l] ? l : level;
    const int s = a.strides[level], ws = a.in_w / s, local = i - a.first[level];
    const float gx = (float)(local % ws), gy = (float)(local / ws), fs = (float)s;
    cx = (cx + gx) * fs, cy = (cy + gy) * fs;
    w = exp32(w) * fs, h = exp32(h) * fs;
  }
  const float hw = w * 0.5f, hh = h * 0.5f;
  const float x1 = (cx - hw) / a.ratio, y1 = (cy - hh) / a.ratio, x2 = (cx + hw) / a.ratio, y2 = (cy + hh) / a.ratio;
  const float score = o[4] * o[a.cls];
  const bool ok = isfinite(score) && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && score > a.threshold;
  float* __restrict__ sc = a.scratch + (size_t)f * 5 * a.A + i;
  sc[0] = ok ? score : 0.f;
  sc[a.A] = x1, sc[2 * (size_t)a.A] = y1, sc[3 * (size_t)a.A] = x2, sc[4 * (size_t)a.A] = y2;
}

struct NmsArgs {
  const float* scratch;                  // [F][5][A]
  float* boxes;                          // [F][P][5]
  int* count;                            // [F]
  int A, people;
  float iou_threshold;
};

__device__ __forceinline__ unsigned long long max_across(unsigned long long key, int width) {
  for (int off = width >> 1; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off, WAVE);
    key = other > key ? other : key;
  }
  return key;
}

// pose_estimate_reference.iou of the emitted box (a) with one other; min / max are selects
__device__ __forceinline__ float iou(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2, float by2) {
  const float area_a = (ax2 - ax1 + 1.f) * (ay2 - ay1 + 1.f);
  const float area_b = (bx2 - bx1 + 1.f) * (by2 - by1 + 1.f);
  float iw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1) + 1.f;
  float ih = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1) + 1.f;
  iw = iw > 0.f ? iw : 0.f, ih = ih > 0.f ? ih : 0.f;
  const float inter = iw * ih;
  return inter / (area_a + area_b - inter);
}

__global__ __launch_bounds__(NMS_THREADS) void pose_boxes_nms_kernel(NmsArgs a) {
  __shared__ unsigned long long wave_key[NMS_WAVES];
  const int t = threadIdx.x, f = blockIdx.x, A = a.A;
  const float* __restrict__ sc = a.scratch + (size_t)f * 5 * A;
  unsigned alive = 0;                                     // bit j: anchor t + 1024 j is a live candidate
#pragma unroll
  for (int j = 0; j < NMS_PER; ++j) {
    const int i = t + j * NMS_THREADS;
    alive |= i < A && sc[i] > 0.f ? 1u << j : 0u;
  }
  float* __restrict__ out = a.boxes + (size_t)f * a.people * 5;
  int n = 0;
  for (; n < a.people; ++n) {
    // a candidate's score is positive, so its bits order as it does; ~anchor makes the lowest anchor win a tie
    unsigned long long key = 0;
    for (unsigned m = alive; m; m &= m - 1) {
      const int i = t + (__ffs(m) - 1) * NMS_THREADS;
      const unsigned long long k = (unsigned long long)__float_as_uint(sc[i]) << 32 | ~(unsigned)i;
      key = k > key ? k : key;
    }
    key = max_across(key, WAVE);
    if ((t & (WAVE - 1)) == 0) wave_key[t / WAVE] = key;
    __syncthreads();
    key = max_across(wave_key[t & (NMS_WAVES - 1)], NMS_WAVES);
    __syncthreads();                                      // wave_key is free for the next round
    if (key >> 32 == 0) break;                            // no live candidate left: the same in every lane
    const int w = (int)~(unsigned)key;                    // < A: it came from a live anchor
    const float wx1 = sc[A + w], wy1 = sc[2 * (size_t)A + w], wx2 = sc[3 * (size_t)A + w], wy2 = sc[4 * (size_t)A + w];
    if (t == 0) out[n * 5] = wx1, out[n * 5 + 1] = wy1, out[n * 5 + 2] = wx2, out[n * 5 + 3] = wy2, out[n * 5 + 4] = __uint_as_float((unsigned)(key >> 32));
    for (unsigned m = alive; m; m &= m - 1) {
      const int j = __ffs(m) - 1, i = t + j * NMS_THREADS;
      const float v = iou(wx1, wy1, wx2, wy2, sc[A + i], sc[2 * (size_t)A + i], sc[3 * (size_t)A + i], sc[4 * (size_t)A + i]);
      alive &= v > a.iou_threshold || i == w ? ~(1u << j) : ~0u;
    }
  }
  if (t == 0) {
    a.count[f] = n;
    for (int r = n; r < a.people; ++r) out[r * 5] = -1.f, out[r * 5 + 1] = -1.f, out[r * 5 + 2] = -1.f, out[r * 5 + 3] = -1.f, out[r * 5 + 4] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------ 2 crops
struct CropArgs {
  const uint8_t* frames;
  const float* boxes;                    // [F][P][5]
  const int* count;                      // [F]
  void* out;                             // [F * P][3][out_h][out_w]
  long frame_stride, chan_stride, pix_stride;             // element (n, c, y, x) of frames at n * frame + c * chan + (y * W + x) * pix
  int people, H, W, out_h, out_w, bgr;
  float padding, mean[3], std[3];
};

// Q values next to each other, Q * sizeof(T)-aligned where Q = 4
template <int Q>
__device__ __forceinline__ void put(float* p, const float (&v)[Q]) {
  if constexpr (Q == 4) *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}
template <int Q>
__device__ __forceinline__ void put(bf16_t* p, const float (&v)[Q]) {
  if constexpr (Q == 4) *(bf16x4*)p = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
  else *p = f2bf(v[0]);
}

// A lane makes Q pixels of one row (Q = 4 where the rows are whole quads and `out` is 16-byte aligned: one vector store
// per channel; Q = 1 otherwise).
template <typename T, int Q>
__global__ __launch_bounds__(CROP_THREADS) void pose_crop_kernel(CropArgs a) {
  const int n = blockIdx.x, px = (blockIdx.y * CROP_THREADS + threadIdx.x) * Q, plane = a.out_h * a.out_w;
  if (px >= plane) return;
  T* __restrict__ o = (T*)a.out + (size_t)n * 3 * plane + px;
  const Window win = window_of(a.boxes, a.count, n, a.people, a.out_h, a.out_w, a.padding);
  float v[3][Q];
  if (!win.valid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int q = 0; q < Q; ++q) v[c][q] = 0.f;
      put<Q>(o + (size_t)c * plane, v[c]);
    }
    return;
  }
  const int j = px / a.out_w, i0 = px - j * a.out_w;
  const float sy = win.cy + ((float)j - (float)a.out_h * 0.5f) * win.ay;
  const uint8_t* __restrict__ src = a.frames + (size_t)(n / a.people) * a.frame_stride;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const float sx = win.cx + ((float)(i0 + q) - (float)a.out_w * 0.5f) * win.ax;
    const bool inside = sx >= -1.f && sx <= (float)a.W && sy >= -1.f && sy <= (float)a.H;
    const float fx0 = floorf(inside ? sx : 0.f), fy0 = floorf(inside ? sy : 0.f);
    const float fx = sx - fx0, fy = sy - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;               // -1 .. W, -1 .. H
    const bool xa = x0 >= 0 && x0 < a.W, xb = x0 + 1 >= 0 && x0 + 1 < a.W, ya = y0 >= 0 && y0 < a.H, yb = y0 + 1 >= 0 && y0 + 1 < a.H;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float s = 0.f;
      asm volatile("" : "+v"(s));                         // an opaque +0: the compiler otherwise turns 0 - mean into -mean, which is -0 for mean = 0
      if (inside) {
        const uint8_t* __restrict__ ch = src + (size_t)(a.bgr ? 2 - c : c) * a.chan_stride;
        const float p00 = ya && xa ? (float)ch[((size_t)y0 * a.W + x0) * a.pix_stride] : 0.f;
        const float p01 = ya && xb ? (float)ch[((size_t)y0 * a.W + x0 + 1) * a.pix_stride] : 0.f;
        const float p10 = yb && xa ? (float)ch[((size_t)(y0 + 1) * a.W + x0) * a.pix_stride] : 0.f;
        const float p11 = yb && xb ? (float)ch[((size_t)(y0 + 1) * a.W + x0 + 1) * a.pix_stride] : 0.f;
        const float top = p00 + (p01 - p00) * fx, bottom = p10 + (p11 - p10) * fx;
        s = top + (bottom - top) * fy;
      }
      v[c][q] = (s - a.mean[c]) / a.std[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) put<Q>(o + (size_t)c * plane, v[c]);
}

// ------------------------------------------------------------------------------------------ 3 keypoints
struct SimccArgs {
  const void* sx;                        // [N][133][Wx]
  const void* sy;                        // [N][133][Wy]
  const float* boxes;                    // [F][P][5]
  const int* count;                      // [F]
  float* out;                            // [N][134][3]
  int people, H, W, Wx, Wy, out_h, out_w, normalized;
  float padding, split_ratio, neck_threshold;
  uint8_t order[POINTS + 2];             // out[i] = tmp[order[i]]
};

struct Best {
  float v;
  int i;
};

__device__ __forceinline__ void take(Best& b, float v, int i, bool in) { b = in && v > b.v ? Best{v, i} : b; }

// The first index of the maximum of one row over its non-NaN entries.  `scan_lane`: a lane scans its own entries upward
// with > (NaN never wins).  VEC entries per load; a load that runs past the row is made at the row's last vector and not
// looked at.  ONE: the row fits one batch of loads (vecs <= 64 * SIMCC_BATCH), so there is no loop, and the loads of the
// rows a wave scans one after the other stand in straight-line code, where the compiler issues them ahead of their use.
template <typename T, int VEC, bool ONE>
__device__ __forceinline__ Best scan_lane(const T* __restrict__ row, int width, int lane) {
  struct alignas(sizeof(T) * VEC) Pack { T e[VEC]; };
  Best b = {-INFINITY, 0};
  const int vecs = width / VEC;                           // VEC = 1, or width is a multiple of VEC
  for (int base = 0; base < (ONE ? 1 : vecs); base += WAVE * SIMCC_BATCH) {
    Pack p[SIMCC_BATCH];
#pragma unroll
    for (int u = 0; u < SIMCC_BATCH; ++u) {
      const int at = base + u * WAVE + lane;
      p[u] = ((const Pack*)row)[at < vecs ? at : vecs - 1];
    }
#pragma unroll
    for (int u = 0; u < SIMCC_BATCH; ++u) {
      const int at = base + u * WAVE + lane;
#pragma unroll
      for (int e = 0; e < VEC; ++e) take(b, (float)p[u].e[e], at * VEC + e, at < vecs);
    }
  }
  return b;
}

// `merge_wave`: the lanes merge, the larger value winning and the lower index on equal values; the result in every lane
__device__ __forceinline__ Best merge_wave(Best b) {
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const float ov = __shfl_xor(b.v, off, WAVE);
    const int oi = __shfl_xor(b.i, off, WAVE);
    b = ov > b.v || (ov == b.v && oi < b.i) ? Best{ov, oi} : b;
  }
  return b;
}

// The rows wave, wave + 16, ... of person n, SIMCC_GROUP at a time: every lane's scans of a group first, then its merges,
// so that the loads of a group are in flight together and the merges do not wait for them one by one.
template <typename T, int VEC, bool ONE>
__device__ __forceinline__ void scan_rows(const SimccArgs& a, int n, int wave, int lane, float* best_v, int* best_i) {
#pragma unroll
  for (int g = 0; g < SIMCC_ROWS; g += SIMCC_GROUP) {
    Best part[SIMCC_GROUP];
#pragma unroll
    for (int q = 0; q < SIMCC_GROUP && g + q < SIMCC_ROWS; ++q) {
      const int r = min(wave + (g + q) * SIMCC_WAVES, 2 * SIMCC - 1);     // past the last row: that row once more, not stored
      const bool is_y = r >= SIMCC;
      const int k = is_y ? r - SIMCC : r, width = is_y ? a.Wy : a.Wx;
      part[q] = scan_lane<T, VEC, ONE>((const T*)(is_y ? a.sy : a.sx) + ((size_t)n * SIMCC + k) * width, width, lane);
    }
#pragma unroll
    for (int q = 0; q < SIMCC_GROUP && g + q < SIMCC_ROWS; ++q) {
      const int r = wave + (g + q) * SIMCC_WAVES;
      const Best b = merge_wave(part[q]);
      if (lane == 0 && r < 2 * SIMCC) best_v[r] = b.v, best_i[r] = b.i;
    }
  }
}

struct Point {
  float x, y, s;
  bool ok;
};

template <typename T>
__global__ __launch_bounds__(SIMCC_THREADS) void pose_simcc_kernel(SimccArgs a) {
  __shared__ float best_v[2 * SIMCC];
  __shared__ int best_i[2 * SIMCC];
  const int n = blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
  float* __restrict__ out = a.out + (size_t)n * POINTS * 3;
  const Window win = window_of(a.boxes, a.count, n, a.people, a.out_h, a.out_w, a.padding);
  if (!win.valid) {                                       // the same in every lane: nothing of the logits is read
    if (t < POINTS) out[t * 3] = ABSENT_XY, out[t * 3 + 1] = ABSENT_XY, out[t * 3 + 2] = ABSENT_SCORE;
    return;
  }
  constexpr int VEC = 16 / sizeof(T), BATCH = WAVE * SIMCC_BATCH;
  const bool wide = a.Wx % VEC == 0 && a.Wy % VEC == 0 && (uintptr_t)a.sx % 16 == 0 && (uintptr_t)a.sy % 16 == 0;   // 16-byte loads in both
  const int most = a.Wx > a.Wy ? a.Wx : a.Wy;
  if (wide && most <= BATCH * VEC) scan_rows<T, VEC, true>(a, n, wave, lane, best_v, best_i);
  else if (wide) scan_rows<T, VEC, false>(a, n, wave, lane, best_v, best_i);
  else if (most <= BATCH) scan_rows<T, 1, true>(a, n, wave, lane, best_v, best_i);
  else scan_rows<T, 1, false>(a, n, wave, lane, best_v, best_i);
  __syncthreads();
  if (t >= POINTS) return;
  auto point = [&](int k) {
    const float mx = best_v[k], my = best_v[SIMCC + k];
    Point p;
    p.s = mx < my ? mx : my;
    p.ok = isfinite(p.s) && p.s > 0.f;
    const float u = (float)best_i[k] / a.split_ratio, v = (float)best_i[SIMCC + k] / a.split_ratio;
    p.x = win.cx + (u - (float)a.out_w * 0.5f) * win.ax;
    p.y = win.cy + (v - (float)a.out_h * 0.5f) * win.ay;
    if (a.normalized) p.x = p.x / (float)a.W, p.y = p.y / (float)a.H;
    return p;
  };
  const int src = a.order[t];                             // an index into tmp: 17 body points, the neck, the other 116
  Point p;
  if (src == 17) {
    const Point l = point(5), r = point(6);
    p.ok = l.ok && r.ok && l.s > a.neck_threshold && r.s > a.neck_threshold;
    p.x = (l.x + r.x) * 0.5f, p.y = (l.y + r.y) * 0.5f, p.s = 1.f;
  } else {
    p = point(src < 17 ? src : src - 1);
  }
  out[t * 3] = p.ok ? p.x : ABSENT_XY, out[t * 3 + 1] = p.ok ? p.y : ABSENT_XY, out[t * 3 + 2] = p.ok ? p.s : ABSENT_SCORE;
}

// ------------------------------------------------------------------------------------------ host
inline int check_people_frames(const char* who, int F, int P) {
  SF_CHECK(F > 0 && F <= SF_POSE_BOXES_MAX_FRAMES, "%s: F=%d (1..%d)", who, F, SF_POSE_BOXES_MAX_FRAMES);
  SF_CHECK(P > 0 && P <= SF_POSE_RENDER_MAX_PEOPLE, "%s: P=%d (1..%d)", who, P, SF_POSE_RENDER_MAX_PEOPLE);
  return 0;
}

inline int check_crop_geometry(const char* who, int H, int W, int out_h, int out_w, float padding) {
  SF_CHECK(H > 0 && H <= SF_POSE_CROP_MAX_FRAME && W > 0 && W <= SF_POSE_CROP_MAX_FRAME, "%s: frames of %d x %d (1..%d)", who, H, W, SF_POSE_CROP_MAX_FRAME);
  SF_CHECK(out_h > 0 && out_h <= SF_POSE_CROP_MAX_SIZE && out_w > 0 && out_w <= SF_POSE_CROP_MAX_SIZE, "%s: out_size %d x %d (1..%d)", who, out_h,
           out_w, SF_POSE_CROP_MAX_SIZE);
  SF_CHECK(std::isfinite(padding) && padding > 0.f, "%s: padding must be finite and > 0", who);
  return 0;
}

}  // namespace

extern "C" size_t sf_pose_boxes_scratch_bytes(int F, int A) {
  return F > 0 && F <= SF_POSE_BOXES_MAX_FRAMES && A > 0 && A <= SF_POSE_BOXES_MAX_ANCHORS ? (size_t)F * A * 5 * sizeof(float) : 0;
}

extern "C" int sf_pose_boxes_decode(const sf_pose_boxes_args* args, void* stream) {
  const char* who = "sf_pose_boxes_decode";
  SF_CHECK(args, "%s: null args", who);
  SF_CHECK(args->head && args->boxes && args->count && args->scratch, "%s: null buffer", who);
  SF_TRY(check_people_frames(who, args->F, args->P));
  SF_CHECK(args->C > 0 && args->C <= SF_POSE_BOXES_MAX_CLASSES, "%s: C=%d (1..%d)", who, args->C, SF_POSE_BOXES_MAX_CLASSES);
  SF_CHECK(args->class_index >= 0 && args->class_index < args->C, "%s: class_index=%d (0..%d)", who, args->class_index, args->C - 1);
  SF_CHECK(args->n_strides > 0 && args->n_strides <= SF_POSE_BOXES_MAX_STRIDES, "%s: n_strides=%d (1..%d)", who, args->n_strides,
           SF_POSE_BOXES_MAX_STRIDES);
  SF_CHECK(args->in_h > 0 && args->in_w > 0 && args->in_h <= (1 << 20) && args->in_w <= (1 << 20), "%s: input_size %d x %d", who, args->in_h, args->in_w);
  CandArgs c;
  long anchors = 0;
  for (int l = 0; l < SF_POSE_BOXES_MAX_STRIDES; ++l) {
    c.strides[l] = 1, c.first[l] = 0;
    if (l >= args->n_strides) continue;
    const int s = args->strides[l];
    SF_CHECK(s > 0 && args->in_h % s == 0 && args->in_w % s == 0, "%s: stride %d does not divide the input size %d x %d", who, s, args->in_h, args->in_w);
    c.strides[l] = s, c.first[l] = (int)anchors;
    anchors += (long)(args->in_h / s) * (args->in_w / s);
    SF_CHECK(anchors <= SF_POSE_BOXES_MAX_ANCHORS, "%s: more than %d anchors", who, SF_POSE_BOXES_MAX_ANCHORS);
  }
  SF_CHECK(args->A == anchors, "%s: A=%d, the input size and the strides give %ld", who, args->A, anchors);
  SF_CHECK(std::isfinite(args->ratio) && args->ratio > 0.f, "%s: ratio must be finite and > 0", who);
  SF_CHECK(std::isfinite(args->score_threshold) && args->score_threshold >= 0.f, "%s: score_threshold must be finite and >= 0", who);
  SF_CHECK(std::isfinite(args->iou_threshold), "%s: iou_threshold must be finite", who);
  SF_CHECK((uintptr_t)args->head % 4 == 0 && (uintptr_t)args->boxes % 4 == 0 && (uintptr_t)args->count % 4 == 0 && (uintptr_t)args->scratch % 4 == 0,
           "%s: head, boxes, count and scratch must be 4-byte aligned", who);
  const int row = 5 + args->C;
  const Range range[4] = {{"head", args->head, (size_t)args->F * args->A * row * sizeof(float)},
                          {"boxes", args->boxes, (size_t)args->F * args->P * 5 * sizeof(float)},
                          {"count", args->count, (size_t)args->F * sizeof(int32_t)},
                          {"scratch", args->scratch, sf_pose_boxes_scratch_bytes(args->F, args->A)}};
  SF_TRY(disjoint(who, range));
  c.head = args->head, c.scratch = args->scratch, c.A = args->A, c.row = row, c.cls = 5 + args->class_index;
  c.in_w = args->in_w, c.n_strides = args->n_strides, c.decoded = args->decoded != 0;
  c.ratio = args->ratio, c.threshold = args->score_threshold;
  SF_TRY(sf_launch<&pose_boxes_candidates_kernel>(who, dim3((unsigned)((args->A + CAND_THREADS - 1) / CAND_THREADS), (unsigned)args->F), dim3(CAND_THREADS),
                                                  0, (hipStream_t)stream, c));
  NmsArgs m;
  m.scratch = args->scratch, m.boxes = args->boxes, m.count = args->count, m.A = args->A, m.people = args->P, m.iou_threshold = args->iou_threshold;
  return sf_launch<&pose_boxes_nms_kernel>(who, dim3((unsigned)args->F), dim3(NMS_THREADS), 0, (hipStream_t)stream, m);
}

extern "C" int sf_pose_crop_people(const sf_pose_crop_args* args, void* stream) {
  const char* who = "sf_pose_crop_people";
  SF_CHECK(args, "%s: null args", who);
  SF_CHECK(args->frames && args->boxes && args->count && args->out, "%s: null buffer", who);
  SF_TRY(check_people_frames(who, args->F, args->P));
  SF_TRY(check_crop_geometry(who, args->H, args->W, args->out_h, args->out_w, args->padding));
  SF_CHECK(args->layout >= SF_JPEG_HWC && args->layout <= SF_JPEG_CHW, "%s: layout=%d (enum sf_jpeg_layout)", who, args->layout);
  SF_CHECK(args->dtype == SF_JPEG_F32 || args->dtype == SF_JPEG_BF16, "%s: dtype=%d (SF_JPEG_F32 or SF_JPEG_BF16)", who, args->dtype);
  for (int c = 0; c < 3; ++c) {
    SF_CHECK(std::isfinite(args->mean[c]), "%s: mean must be finite", who);
    SF_CHECK(std::isfinite(args->std[c]) && args->std[c] > 0.f, "%s: std must be finite and > 0", who);
  }
  const size_t elem = args->dtype == SF_JPEG_F32 ? 4 : 2;
  SF_CHECK((uintptr_t)args->boxes % 4 == 0 && (uintptr_t)args->count % 4 == 0 && (uintptr_t)args->out % elem == 0,
           "%s: boxes and count must be 4-byte aligned, out to its element", who);
  const size_t pixels = (size_t)args->H * args->W, plane = (size_t)args->out_h * args->out_w;
  const Range range[4] = {{"frames", args->frames, (size_t)args->F * 3 * pixels},
                          {"boxes", args->boxes, (size_t)args->F * args->P * 5 * sizeof(float)},
                          {"count", args->count, (size_t)args->F * sizeof(int32_t)},
                          {"out", args->out, (size_t)args->F * args->P * 3 * plane * elem}};
  SF_TRY(disjoint(who, range));
  CropArgs a;
  a.frames = (const uint8_t*)args->frames, a.boxes = args->boxes, a.count = args->count, a.out = args->out;
  const FrameStrides from = frame_strides(args->layout, args->F, args->H, args->W);
  a.frame_stride = from.sn, a.chan_stride = from.sc, a.pix_stride = from.sx;
  a.people = args->P, a.H = args->H, a.W = args->W, a.out_h = args->out_h, a.out_w = args->out_w, a.bgr = args->bgr != 0;
  a.padding = args->padding;
  for (int c = 0; c < 3; ++c) a.mean[c] = args->mean[c], a.std[c] = args->std[c];
  const bool quads = args->out_w % 4 == 0 && (uintptr_t)args->out % 16 == 0;          // a row is whole quads, and every quad is aligned
  const size_t lanes = quads ? plane / 4 : plane;
  const dim3 grid((unsigned)(args->F * args->P), (unsigned)((lanes + CROP_THREADS - 1) / CROP_THREADS));
  const hipStream_t s = (hipStream_t)stream;
  return pixel_dispatch<false>(args->dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return quads ? sf_launch<&pose_crop_kernel<T, 4>>(who, grid, dim3(CROP_THREADS), 0, s, a) : sf_launch<&pose_crop_kernel<T, 1>>(who, grid, dim3(CROP_THREADS), 0, s, a);
  });
}

extern "C" int sf_pose_simcc_decode(const sf_pose_simcc_args* args, void* stream) {
  const char* who = "sf_pose_simcc_decode";
  SF_CHECK(args, "%s: null args", who);
  SF_CHECK(args->simcc_x && args->simcc_y && args->boxes && args->count && args->out && args->order, "%s: null buffer", who);
  SF_TRY(check_people_frames(who, args->F, args->P));
  SF_TRY(check_crop_geometry(who, args->H, args->W, args->out_h, args->out_w, args->padding));
  SF_CHECK(args->Wx > 0 && args->Wx <= SF_POSE_SIMCC_MAX_BINS && args->Wy > 0 && args->Wy <= SF_POSE_SIMCC_MAX_BINS, "%s: bins %d and %d (1..%d)", who,
           args->Wx, args->Wy, SF_POSE_SIMCC_MAX_BINS);
  SF_CHECK(args->dtype == SF_POSE_SIMCC_F32 || args->dtype == SF_POSE_SIMCC_F16, "%s: dtype=%d (enum sf_pose_simcc_dtype)", who, args->dtype);
  SF_CHECK(std::isfinite(args->split_ratio) && args->split_ratio > 0.f, "%s: split_ratio must be finite and > 0", who);
  SF_CHECK(std::isfinite(args->neck_threshold), "%s: neck_threshold must be finite", who);
  const size_t elem = args->dtype == SF_POSE_SIMCC_F32 ? 4 : 2;
  SF_CHECK((uintptr_t)args->simcc_x % elem == 0 && (uintptr_t)args->simcc_y % elem == 0, "%s: simcc_x and simcc_y must be aligned to their element", who);
  SF_CHECK((uintptr_t)args->boxes % 4 == 0 && (uintptr_t)args->count % 4 == 0 && (uintptr_t)args->out % 4 == 0,
           "%s: boxes, count and out must be 4-byte aligned", who);
  SimccArgs a;
  for (int i = 0; i < POINTS; ++i) {
    SF_CHECK(args->order[i] < POINTS, "%s: order[%d]=%d (0..%d)", who, i, args->order[i], POINTS - 1);
    a.order[i] = args->order[i];
  }
  a.order[POINTS] = a.order[POINTS + 1] = 0;
  const size_t people = (size_t)args->F * args->P;
  const Range range[5] = {{"simcc_x", args->simcc_x, people * SIMCC * args->Wx * elem},
                          {"simcc_y", args->simcc_y, people * SIMCC * args->Wy * elem},
                          {"boxes", args->boxes, people * 5 * sizeof(float)},
                          {"count", args->count, (size_t)args->F * sizeof(int32_t)},
                          {"out", args->out, people * POINTS * 3 * sizeof(float)}};
  SF_TRY(disjoint(who, range));
  a.sx = args->simcc_x, a.sy = args->simcc_y, a.boxes = args->boxes, a.count = args->count, a.out = args->out;
  a.people = args->P, a.H = args->H, a.W = args->W, a.Wx = args->Wx, a.Wy = args->Wy, a.out_h = args->out_h, a.out_w = args->out_w;
  a.normalized = args->normalized != 0;
  a.padding = args->padding, a.split_ratio = args->split_ratio, a.neck_threshold = args->neck_threshold;
  const dim3 grid((unsigned)people);
  if (args->dtype == SF_POSE_SIMCC_F32) return sf_launch<&pose_simcc_kernel<float>>(who, grid, dim3(SIMCC_THREADS), 0, (hipStream_t)stream, a);
  return sf_launch<&pose_simcc_kernel<_Float16>>(who, grid, dim3(SIMCC_THREADS), 0, (hipStream_t)stream, a);
}
