// Pose renderer (gfx950): DWPose whole-body keypoints become skeleton frames on the device.  The definition of every
// pixel is self_forcing_amd/pose_render_reference.py (`quantize`, `primitives`, `inside`): integer coverage tests of
// ellipses (limbs), discs (joints, hand and face points) and capsules (hand edges), painted in a fixed order.  This file
// equals it bit for bit.
//
// One launch for a whole group of frames, one workgroup of 256 threads per tile of TH x TW pixels of one frame:
//   phase 1  the lanes share out the frame's 185 * P primitives in passes of 256: each lane decodes its primitive's
//            kind, points, radius and colour from the index, quantises and validates the points, forms the bounding box
//            (pose_render_reference.extent) and tests it against the tile.  The hits are compacted into LDS in painter's
//            order: a wave64 ballot and the popcount of the lanes below within a wave, the waves' counts (one LDS slot
//            per pass and wave) across waves.  The list holds every primitive of SF_POSE_RENDER_MAX_PEOPLE people, so it
//            cannot overflow.
//   phase 2  each lane owns four neighbouring pixels of one row and walks the list from the back: the first primitive
//            that covers a pixel decides it, and the lane leaves once all four are decided.  All lanes read the same list
//            entry (an LDS broadcast).  A lane skips a primitive whose box misses its quad before any multiply; the 64-bit
//            products (u^2, v^2 L2, L2^2 of the ellipse, c^2 of the capsule) are formed only behind that, everything else
//            is int32, whose ranges the reference's docstring gives.  An empty list stores zeros.
// Every read of the keypoints lies inside [F][P][134][3]; every write inside the tile and the frame (store_rgb4 drops the
// columns >= W).
#include <cmath>
#include "sf_frame_host.h"
#include "pixel_format.h"

namespace {

constexpr int TW = 64, TH = 16;                      // tile; 256 threads = TH rows x TW / 4 quads
constexpr int PER_PERSON = 185;
constexpr int LIST = PER_PERSON * SF_POSE_RENDER_MAX_PEOPLE;
constexpr int PASSES = (LIST + 255) / 256;
constexpr int LIMB = 0, DISC = 1, EDGE = 2;
constexpr int FACE0 = 24, LEFT0 = 92, RIGHT0 = 113;

#define RGB(r, g, b) ((uint32_t)(r) | ((uint32_t)(g) << 8) | ((uint32_t)(b) << 16))
#define DIM(r, g, b) RGB((r) * 3 / 5, (g) * 3 / 5, (b) * 3 / 5)
__constant__ const uint8_t LIMB_A[17] = {1, 1, 2, 3, 5, 6, 1, 8, 9, 1, 11, 12, 1, 0, 14, 0, 15};
__constant__ const uint8_t LIMB_B[17] = {2, 5, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 0, 14, 16, 15, 17};
__constant__ const uint32_t COLORS[18] = {RGB(255, 0, 0),   RGB(255, 85, 0),  RGB(255, 170, 0), RGB(255, 255, 0), RGB(170, 255, 0), RGB(85, 255, 0),
                                          RGB(0, 255, 0),   RGB(0, 255, 85),  RGB(0, 255, 170), RGB(0, 255, 255), RGB(0, 170, 255), RGB(0, 85, 255),
                                          RGB(0, 0, 255),   RGB(85, 0, 255),  RGB(170, 0, 255), RGB(255, 0, 255), RGB(255, 0, 170), RGB(255, 0, 85)};
__constant__ const uint32_t LIMB_COLORS[17] = {DIM(255, 0, 0),   DIM(255, 85, 0),  DIM(255, 170, 0), DIM(255, 255, 0), DIM(170, 255, 0), DIM(85, 255, 0),
                                               DIM(0, 255, 0),   DIM(0, 255, 85),  DIM(0, 255, 170), DIM(0, 255, 255), DIM(0, 170, 255), DIM(0, 85, 255),
                                               DIM(0, 0, 255),   DIM(85, 0, 255),  DIM(170, 0, 255), DIM(255, 0, 255), DIM(255, 0, 170)};
__constant__ const uint8_t HAND_A[20] = {0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19};
__constant__ const uint8_t HAND_B[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20};
// int(255 * channel) of colorsys.hsv_to_rgb(e / 20, 1, 1) (pose_render_reference.HAND_EDGE_COLORS)
__constant__ const uint32_t HAND_EDGE_COLORS[20] = {RGB(255, 0, 0),   RGB(255, 76, 0),  RGB(255, 153, 0), RGB(255, 229, 0), RGB(203, 255, 0),
                                                    RGB(127, 255, 0), RGB(51, 255, 0),  RGB(0, 255, 25),  RGB(0, 255, 102), RGB(0, 255, 178),
                                                    RGB(0, 255, 255), RGB(0, 178, 255), RGB(0, 102, 255), RGB(0, 25, 255),  RGB(50, 0, 255),
                                                    RGB(127, 0, 255), RGB(204, 0, 255), RGB(255, 0, 229), RGB(255, 0, 152), RGB(255, 0, 76)};

struct RenderArgs {
  const float* kp;                       // [F][P][134][3]
  int P, H, W;
  int normalized;
  float threshold;
  long sn, sc, sy, sx;                   // element strides of the output's frame, channel, row, column
};

struct Prim {
  int kind, a, b, r, person;             // a, b: indices of the two points (a == b for a disc)
  uint32_t color;
};

// primitive k of a frame of P people in painter's order (pose_render_reference.primitives)
__device__ __forceinline__ Prim decode(int k, int P) {
  Prim p;
  p.r = 0;
  if (k < 17 * P) {
    const int i = k / P;
    p.kind = LIMB, p.person = k - i * P, p.a = LIMB_A[i], p.b = LIMB_B[i], p.color = LIMB_COLORS[i];
  } else if (k < 35 * P) {
    k -= 17 * P;
    const int j = k / P;
    p.kind = DISC, p.person = k - j * P, p.a = p.b = j, p.r = 4, p.color = COLORS[j];
  } else if (k < 117 * P) {
    k -= 35 * P;
    p.person = k / 82;
    const int e = k - p.person * 82, base = e < 41 ? LEFT0 : RIGHT0, h = e < 41 ? e : e - 41;
    if (h < 20) {
      p.kind = EDGE, p.a = base + HAND_A[h], p.b = base + HAND_B[h], p.color = HAND_EDGE_COLORS[h];
    } else {
      p.kind = DISC, p.a = p.b = base + h - 20, p.r = 4, p.color = RGB(0, 0, 255);
    }
  } else {
    k -= 117 * P;
    p.person = k / 68;
    p.kind = DISC, p.a = p.b = FACE0 + k - p.person * 68, p.r = 3, p.color = RGB(255, 255, 255);
  }
  return p;
}

// (x, y, score) -> pixel and validity (pose_render_reference.quantize)
__device__ __forceinline__ bool quantize(const float* pt, const RenderArgs& a, int& X, int& Y) {
  const float x = pt[0], y = pt[1], s = pt[2];
  X = Y = 0;
  if (!(isfinite(x) && isfinite(y) && isfinite(s)) || !(s >= a.threshold) || !(x >= 0.f && y >= 0.f)) return false;
  const float px = a.normalized ? x * (float)a.W : x, py = a.normalized ? y * (float)a.H : y;
  if (!(px < (float)(SF_POSE_RENDER_MAX_COORD + 1) && py < (float)(SF_POSE_RENDER_MAX_COORD + 1))) return false;
  X = (int)px, Y = (int)py;
  return true;
}

// pose_render_reference.inside at the pixel centre (px, py)
__device__ __forceinline__ bool covers(int kind, int ax, int ay, int bx, int by, int r, int px, int py) {
  const int ex = px - ax, ey = py - ay;
  if (kind == DISC) return ex * ex + ey * ey <= r * r + r;
  const int dx = bx - ax, dy = by - ay, L2 = dx * dx + dy * dy;
  if (kind == LIMB) {
    const int qx = 2 * px - (ax + bx), qy = 2 * py - (ay + by);
    const long u = qx * dx + qy * dy, v = qx * dy - qy * dx, l = L2;
    const long uu = u * u, vv = v * v, ll = l * l;
    if (vv > 64 * l || uu > ll) return false;
    return 64 * uu + vv * l <= 64 * ll;
  }
  const int s = ex * dx + ey * dy;
  if (s <= 0) return ex * ex + ey * ey <= 1;
  if (s >= L2) {
    const int fx = px - bx, fy = py - by;
    return fx * fx + fy * fy <= 1;
  }
  const long c = ex * dy - ey * dx;
  return c * c <= (long)L2;
}

template <typename T>
__global__ __launch_bounds__(256) void pose_render_kernel(RenderArgs a, T* __restrict__ out) {
  __shared__ uint32_t s_list[LIST][3];     // (ax | ay << 16, bx | by << 16, colour | kind << 24 | r << 26)
  __shared__ int s_count[PASSES][4];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tiles_x = (a.W + TW - 1) / TW;
  const int ox0 = (int)(blockIdx.x % tiles_x) * TW, oy0 = (int)(blockIdx.x / tiles_x) * TH;
  const long f = blockIdx.y;
  const int nprim = PER_PERSON * a.P;

  // ---- phase 1: the primitives that reach this tile, in painter's order
  int total = 0;
  for (int pass = 0; pass * 256 < nprim; ++pass) {
    const int k = pass * 256 + t;
    bool hit = false;
    uint32_t w0 = 0, w1 = 0, w2 = 0;
    if (k < nprim) {
      const Prim p = decode(k, a.P);
      const float* pts = a.kp + (f * a.P + p.person) * (long)(POINTS * 3);
      int ax, ay, bx, by;
      const bool va = quantize(pts + 3 * p.a, a, ax, ay), vb = quantize(pts + 3 * p.b, a, bx, by);
      const bool drawn = va && vb && !(p.kind == LIMB && ax == bx && ay == by);
      const int pad = p.kind == LIMB ? 4 : (p.kind == DISC ? p.r : 1);
      hit = drawn && min(ax, bx) - pad < ox0 + TW && max(ax, bx) + pad >= ox0 && min(ay, by) - pad < oy0 + TH && max(ay, by) + pad >= oy0;
      w0 = (uint32_t)ax | ((uint32_t)ay << 16), w1 = (uint32_t)bx | ((uint32_t)by << 16);
      w2 = p.color | ((uint32_t)p.kind << 24) | ((uint32_t)p.r << 26);
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_count[pass][wave] = __popcll(m);
    __syncthreads();
    int at = total;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = s_count[pass][w];
      at += w < wave ? c : 0;
      total += c;
    }
    if (hit) {
      uint32_t* e = s_list[at + __popcll(m & ((1ull << lane) - 1))];
      e[0] = w0, e[1] = w1, e[2] = w2;
    }
  }
  __syncthreads();

  // ---- phase 2: four pixels of one row per lane, the list from the back
  const int y = oy0 + (t >> 4), x0 = ox0 + 4 * (t & 15);
  if (y >= a.H || x0 >= a.W) return;
  int rgb[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  unsigned open = x0 + 3 < a.W ? 15u : (1u << (a.W - x0)) - 1;       // the pixels not decided yet
  for (int j = total - 1; j >= 0 && open; --j) {
    const uint32_t w0 = s_list[j][0], w1 = s_list[j][1], w2 = s_list[j][2];
    const int ax = w0 & 0xffff, ay = w0 >> 16, bx = w1 & 0xffff, by = w1 >> 16;
    const int kind = (w2 >> 24) & 3, r = w2 >> 26;
    const int pad = kind == LIMB ? 4 : (kind == DISC ? r : 1);
    if (y < min(ay, by) - pad || y > max(ay, by) + pad || x0 + 3 < min(ax, bx) - pad || x0 > max(ax, bx) + pad) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if ((open >> i & 1) && covers(kind, ax, ay, bx, by, r, x0 + i, y)) {
        open &= ~(1u << i);
        rgb[0][i] = w2 & 255, rgb[1][i] = (w2 >> 8) & 255, rgb[2][i] = (w2 >> 16) & 255;
      }
  }
  T* o = out + f * a.sn + (long)y * a.sy + (long)x0 * a.sx;
  store_rgb4(o, rgb, x0, a.W, a.sc, a.sx);
}

}  // namespace

extern "C" int sf_pose_render_frames(const sf_pose_render_args* args, void* stream) {
  const char* who = "sf_pose_render_frames";
  SF_CHECK(args, "%s: null args", who);
  SF_CHECK(args->keypoints && args->out, "%s: null buffer", who);
  SF_CHECK(args->F > 0 && args->F <= 65535, "%s: F=%d frames (1..65535)", who, args->F);
  SF_CHECK(args->P > 0 && args->P <= SF_POSE_RENDER_MAX_PEOPLE, "%s: P=%d people (1..%d)", who, args->P, SF_POSE_RENDER_MAX_PEOPLE);
  SF_CHECK(args->H > 0 && args->W > 0 && args->H <= SF_POSE_RENDER_MAX_SIZE && args->W <= SF_POSE_RENDER_MAX_SIZE, "%s: frame %dx%d (1..%d)", who,
           args->H, args->W, SF_POSE_RENDER_MAX_SIZE);
  SF_CHECK(args->layout >= SF_JPEG_HWC && args->layout <= SF_JPEG_CHW, "%s: unknown layout %d", who, args->layout);
  SF_CHECK(args->dtype >= SF_JPEG_U8 && args->dtype <= SF_JPEG_BF16, "%s: unknown dtype %d", who, args->dtype);
  SF_CHECK(args->normalized == 0 || args->normalized == 1, "%s: normalized=%d (0 or 1)", who, args->normalized);
  SF_CHECK(std::isfinite(args->score_threshold), "%s: score_threshold must be finite", who);
  SF_CHECK((uintptr_t)args->keypoints % 4 == 0 && (uintptr_t)args->out % 16 == 0, "%s: keypoints must be 4-byte, out 16-byte aligned", who);
  RenderArgs a;
  a.kp = args->keypoints, a.P = args->P, a.H = args->H, a.W = args->W;
  a.normalized = args->normalized, a.threshold = args->score_threshold;
  const FrameStrides to = frame_strides(args->layout, args->F, a.H, a.W);
  a.sn = to.sn, a.sc = to.sc, a.sy = to.sy, a.sx = to.sx;
  const dim3 grid((unsigned)(((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH)), (unsigned)args->F);
  hipStream_t s = (hipStream_t)stream;
  return pixel_dispatch(args->dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return sf_launch<&pose_render_kernel<T>>(who, grid, dim3(256), 0, s, a, (T*)args->out);
  });
}
