// The narrow-channel 3x3x3 / 3x3 convolution of the pose front end on channels-last bf16 volumes for gfx950 (MI355X).
//
// Replaces, on the pose path of the many-step sampler (pipeline/causal_diffusion_inference.py), the nn.Conv3d layers
// 0..10 of `dwpose_embedding` (:89-101) and the nn.Conv2d layers of `randomref_embedding_pose` (:109-120), each with
// the nn.SiLU behind it, and the input transform in front of them (:337-343: first frame repeated three times,
// `/ 255.0`, layout).  The 16 -> 5120 layer (:102) is a gather (here) + sf_gemm_bf16 (pose_embed.hip).
//
//   out[(t,h,w)][n] = act( bias[n] + sum over taps (dt,dh,dw), ci of
//                          x[t*st - pt + dt][h*ss - 1 + dh][w*ss - 1 + dw][ci] * wk[n][((dt*3 + dh)*3 + dw)*Cin + ci] )
//
// with zero padding on every side (pt = 1 for kt = 3, 0 for kt = 1).  Implicit GEMM with M = output voxels, N = 16 (one
// MFMA column block; 32 for the 20-channel layer) and K = taps * Cin on v_mfma_f32_16x16x32_bf16.  Every other
// convolution of this library needs Cin % 32 == 0; these layers have 3 (stored as 8) and 16 channels on pixel-resolution
// volumes, so they are bound by bytes, and the structure follows from that:
//   * a workgroup owns a brick of TT x TH x 16 output voxels and stages the input brick with its halo in LDS ONCE; all
//     taps are served from it.  A lane's A fragment (8 consecutive k) is 8 channels of one tap = one 16-byte LDS read,
//     no transpose.  With 32-byte voxels the 16 lanes of a ds_read_b128 group touch 16 distinct bank quads.
//   * the whole weight tensor (14 KiB for 16 -> 16) lives in registers as B fragments, 14 x 4 VGPRs per lane, loaded
//     once per workgroup; workgroups are persistent and walk a contiguous run of bricks (w fastest), so the halo shared
//     by consecutive bricks is still in the L2 of the XCD that read it.
//   * fp32 accumulation, fp32 bias, SiLU in fp32, one rounding to bf16; 16 lanes x 4 quarters write 512 contiguous bytes.
// The 3x3x3 layers also run over a temporal WINDOW of a clip (sf_pose_conv_window): x holds a range of the clip's frames,
// the brick walk starts at any output frame, and every output element is formed from the same taps in the same k order
// as in the whole-volume call, so a clip embedded piece by piece has the whole clip's bits.
#include "sf_frame_host.h"

namespace {

constexpr int PTHREADS = 256;
constexpr int TW = 16;   // output voxels along w per MFMA row tile

struct PConvP {
  const char* x;
  const bf16_t* w;
  const float* bias;
  char* out;
  int T, H, W;             // input volume
  int To, Ho, Wo;          // output volume
  int Cout, ldw, ldo, silu;
  int ntw, nth, ntiles, per;   // brick grid (w fastest, then h, then t) and bricks per workgroup
};

template <int CIN, int KT, int ST, int SS>
struct Geo {
  static constexpr int TT = KT == 1 ? 1 : (ST == 1 && SS == 1 ? 4 : 2);
  static constexpr int TH = SS == 1 ? 8 : 4;
  static constexpr int BT = (TT - 1) * ST + KT, BH = (TH - 1) * SS + 3, BW = (TW - 1) * SS + 3;
  static constexpr int VOX = CIN * 2;                 // bytes per voxel
  static constexpr int PPV = CIN / 8;                 // 16-byte pieces per voxel
  static constexpr int NPIECE = BT * BH * BW * PPV;
  static constexpr int LDS_BYTES = NPIECE * 16;
  static constexpr int NTAP = KT * 9;
  static constexpr int TPS = 32 / CIN;                // taps per 32-deep k-step
  static constexpr int NK = (NTAP + TPS - 1) / TPS;
  static constexpr int MT = TT * TH / 4;              // row tiles per wave
  static constexpr int MU = MT >= 2 ? 2 : 1;          // row tiles in flight (independent accumulator chains)
  static constexpr int PT = KT == 3 ? 1 : 0;
  static_assert(LDS_BYTES <= 64 * 1024, "the brick fits the default LDS limit");
  static_assert((TT * TH) % 4 == 0 && MT % MU == 0, "row tiles divide among the four waves");
};

// The temporal window of sf_pose_conv_window: x holds the clip-timeline frames [x_t0, x_t0 + T); a tap is loaded when its
// frame lies in [t_lo, t_hi) (the window clipped to the timeline's valid range) and is a literal zero otherwise; the
// brick walk along t starts at output frame t_out0, which is written at out's start, and p.To counts the frames written.
struct PWin { int x_t0, t_lo, t_hi, t_out0; };

// WIN = false is the whole-volume kernel: x is the timeline [0, T), the walk starts at output frame 0.
template <int CIN, int KT, int ST, int SS, int NB, bool WIN>
__device__ __forceinline__ void pose_conv_body(const PConvP& p, const PWin& pw, char* brick) {
  using G = Geo<CIN, KT, ST, SS>;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m16 = lane & 15, kq = lane >> 4;

  // ---- the resident weights: B fragment of k-step s, column block nb = row (nb*16 + m16) of wk, k = 32 s + 8 kq ..
  bf16x8 wf[G::NK][NB];
#pragma unroll
  for (int s = 0; s < G::NK; ++s)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) wf[s][nb] = *reinterpret_cast<const bf16x8*>(p.w + (long)(nb * 16 + m16) * p.ldw + s * 32 + kq * 8);
  f32x4 bias[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) bias[nb] = *reinterpret_cast<const f32x4*>(p.bias + nb * 16 + kq * 4);

  // ---- byte offset inside the brick of this lane's A piece of k-step s, for the row tile at brick origin: the piece is
  // 8 channels of tap (dt, dh, dw) at output column m16.  A tap past the last one (the zero-weight padding of K) reads
  // offset 0 and is replaced by zeros.
  int aoff[G::NK];
  bool last_pad = false;
#pragma unroll
  for (int s = 0; s < G::NK; ++s) {
    const int tap = CIN == 16 ? 2 * s + (kq >> 1) : 4 * s + kq;
    const int half = CIN == 16 ? (kq & 1) : 0;
    const bool pad = tap >= G::NTAP;
    const int tp = pad ? 0 : tap;
    const int dt = tp / 9, r = tp - 9 * dt, dh = r / 3, dw = r - 3 * dh;
    aoff[s] = (((dt * G::BH + dh) * G::BW) + dw + m16 * SS) * G::VOX + half * 16;
    if (s == G::NK - 1) last_pad = pad;
  }

  // ---- this workgroup's run of bricks: XCD x takes a contiguous eighth of the workgroups' runs
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int lid = (nwg & 7) == 0 ? (bid & 7) * (nwg >> 3) + (bid >> 3) : bid;
  const int tile_end = min((lid + 1) * p.per, p.ntiles);

  for (int tile = lid * p.per; tile < tile_end; ++tile) {
    const int tw_i = tile % p.ntw, r0 = tile / p.ntw;
    const int th_i = r0 % p.nth, tt_i = r0 / p.nth;
    const int t0 = (WIN ? pw.t_out0 : 0) + tt_i * G::TT, h0 = th_i * G::TH, w0 = tw_i * TW;
    const int ti0 = t0 * ST - G::PT, hi0 = h0 * SS - 1, wi0 = w0 * SS - 1;

    // ---- stage the input brick (zeros outside the volume), four 16-byte pieces per thread in flight
    for (int i0 = tid; i0 < G::NPIECE; i0 += 4 * PTHREADS) {
      bf16x8 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i0 + j * PTHREADS;
        const int vx = i / G::PPV, hf = i - vx * G::PPV;
        const int bw = vx % G::BW, r = vx / G::BW;
        const int bh = r % G::BH, bt = r / G::BH;
        const int ti = ti0 + bt, hi = hi0 + bh, wi = wi0 + bw;
        v[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        const bool t_in = WIN ? (ti >= pw.t_lo && ti < pw.t_hi) : ((unsigned)ti < (unsigned)p.T);
        const int tx = WIN ? ti - pw.x_t0 : ti;          // the frame's place in x
        if (i < G::NPIECE && t_in && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) {
          const unsigned off = ((unsigned)((tx * p.H + hi) * p.W + wi) * G::PPV + hf) * 16u;   // < 4 GiB: checked by the host
          v[j] = *reinterpret_cast<const bf16x8*>(p.x + off);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i0 + j * PTHREADS;
        if (i < G::NPIECE) *reinterpret_cast<bf16x8*>(brick + i * 16) = v[j];
      }
    }
    __syncthreads();

#pragma unroll 1
    for (int mt = 0; mt < G::MT; mt += G::MU) {
      f32x4 acc[G::MU][NB];
      int rowb[G::MU];
#pragma unroll
      for (int u = 0; u < G::MU; ++u) {
        const int row = wave * G::MT + mt + u;          // row tile (tt, th) of the brick
        const int tt = row / G::TH, th = row - tt * G::TH;
        rowb[u] = ((tt * ST) * G::BH + th * SS) * G::BW * G::VOX;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[u][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int s = 0; s < G::NK; ++s) {
#pragma unroll
        for (int u = 0; u < G::MU; ++u) {
          bf16x8 xf = *reinterpret_cast<const bf16x8*>(brick + rowb[u] + aoff[s]);
          if (s == G::NK - 1 && last_pad) xf = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[u][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][nb], xf, acc[u][nb], 0, 0, 0);
        }
      }
      // ---- epilogue: the lane holds y[m16][nb*16 + 4 kq .. + 3] of each row tile
#pragma unroll
      for (int u = 0; u < G::MU; ++u) {
        const int row = wave * G::MT + mt + u;
        const int tt = row / G::TH, th = row - tt * G::TH;
        const int t = t0 + tt - (WIN ? pw.t_out0 : 0), h = h0 + th, w = w0 + m16;   // t: the frame's place in out
        if (t >= p.To || h >= p.Ho || w >= p.Wo) continue;
        const unsigned obase = (unsigned)((t * p.Ho + h) * p.Wo + w) * (unsigned)(p.ldo * 2);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int n = nb * 16 + kq * 4;
          if (n >= p.Cout) continue;
          bf16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float y = acc[u][nb][j] + bias[nb][j];
            if (p.silu) y = silu_f(y);
            o[j] = (bf16_t)y;
          }
          *reinterpret_cast<bf16x4*>(p.out + obase + n * 2) = o;
        }
      }
    }
    __syncthreads();   // the brick is free for the next one
  }
}

template <int CIN, int KT, int ST, int SS, int NB>
__global__ __launch_bounds__(PTHREADS) void pose_conv_kernel(PConvP p) {
  __shared__ __attribute__((aligned(16))) char brick[Geo<CIN, KT, ST, SS>::LDS_BYTES];
  pose_conv_body<CIN, KT, ST, SS, NB, false>(p, PWin{0, 0, 0, 0}, brick);
}

template <int CIN, int KT, int ST, int SS, int NB>
__global__ __launch_bounds__(PTHREADS) void pose_conv_window_kernel(PConvP p, PWin pw) {
  __shared__ __attribute__((aligned(16))) char brick[Geo<CIN, KT, ST, SS>::LDS_BYTES];
  pose_conv_body<CIN, KT, ST, SS, NB, true>(p, pw, brick);
}

template <int CIN, int KT, int ST, int SS, int NB>
int launch(PConvP& p, const char* who, hipStream_t s, const PWin* pw = nullptr) {
  using G = Geo<CIN, KT, ST, SS>;
  p.ntw = (p.Wo + TW - 1) / TW;
  p.nth = (p.Ho + G::TH - 1) / G::TH;
  const long ntiles = (long)p.ntw * p.nth * ((p.To + G::TT - 1) / G::TT);
  SF_CHECK(ntiles < (1L << 30), "%s: too many output bricks", who);
  p.ntiles = (int)ntiles;
  int nwg = p.ntiles < 1024 ? p.ntiles : 1024;          // 4 persistent workgroups per CU
  if (nwg >= 8) nwg &= ~7;
  p.per = (p.ntiles + nwg - 1) / nwg;
  nwg = (p.ntiles + p.per - 1) / p.per;                  // no idle workgroups; the XCD remap needs nwg % 8 == 0 and is skipped otherwise
  if constexpr (KT == 3) {      // the window mode exists for the dwpose stack's layers only
    if (pw) return sf_launch<&pose_conv_window_kernel<CIN, KT, ST, SS, NB>>(who, dim3(nwg), dim3(PTHREADS), 0, s, p, *pw);
  }
  return sf_launch<&pose_conv_kernel<CIN, KT, ST, SS, NB>>(who, dim3(nwg), dim3(PTHREADS), 0, s, p);
}

// pose frames / the reference pose image -> channels-last bf16 with 8 stored channels (3 real), `lead` copies of the
// first frame in front, value / 255 (the fp32 quotient rounded once)
template <typename T>
__global__ __launch_bounds__(256) void pose_prepare_kernel(const T* __restrict__ src, bf16_t* __restrict__ out, long n_pos, int hw, long plane, int hwc,
                                                           int lead) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (output frame, position)
  if (i >= n_pos) return;
  const long fo = i / hw, pos = i - fo * hw;
  const long f = fo < lead ? 0 : fo - lead;
  bf16x8 v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T s = hwc ? src[(f * hw + pos) * 3 + c] : src[c * plane + f * hw + pos];
    v[c] = (bf16_t)((float)s / 255.0f);
  }
  *reinterpret_cast<bf16x8*>(out + i * 8) = v;
}

}  // namespace

extern "C" int sf_pose_out_size(int n, int kernel, int stride) {
  // nn.Conv3d / nn.Conv2d output size: kernel 3 with padding 1, or kernel 2 without padding
  if (n <= 0 || stride <= 0) return 0;
  return kernel == 3 ? (n - 1) / stride + 1 : n >= kernel ? (n - kernel) / stride + 1 : 0;
}

namespace {

// The argument checks both entry points share, and the kernel parameters of the whole-volume call.
int conv_setup(const sf_pose_conv_args* a, const char* who, PConvP& p, int& nb) {
  SF_CHECK(a != nullptr, "%s: null args", who);
  SF_CHECK(a->x && a->w && a->bias && a->out, "%s: null tensor", who);
  SF_CHECK(a->T > 0 && a->H > 0 && a->W > 0, "%s: empty volume %dx%dx%d", who, a->T, a->H, a->W);
  SF_CHECK(a->Cin == 8 || a->Cin == 16, "%s: Cin=%d (8 = three channels stored padded, or 16)", who, a->Cin);
  SF_CHECK(a->kt == 1 || a->kt == 3, "%s: kt must be 1 or 3, got %d", who, a->kt);
  SF_CHECK((a->stride_t == 1 || a->stride_t == 2) && (a->stride_s == 1 || a->stride_s == 2), "%s: strides must be 1 or 2, got t=%d s=%d", who,
           a->stride_t, a->stride_s);
  SF_CHECK(a->kt == 3 || a->stride_t == 1, "%s: kt = 1 goes with temporal stride 1", who);
  SF_CHECK(a->Cout > 0 && a->Cout <= 32 && a->Cout % 4 == 0, "%s: Cout=%d (a multiple of 4, at most 32)", who, a->Cout);
  nb = a->Cout <= 16 ? 1 : 2;
  const int tps = 32 / a->Cin, nk = (a->kt * 9 + tps - 1) / tps;
  SF_CHECK(a->ldw >= nk * 32 && a->ldw % 8 == 0, "%s: weight row stride %d < padded K %d", who, a->ldw, nk * 32);
  SF_CHECK(a->ldo >= a->Cout && a->ldo % 4 == 0, "%s: ldo=%d too small for %d channels or not a multiple of 4", who, a->ldo, a->Cout);
  SF_CHECK(((uintptr_t)a->x % 16 == 0) && ((uintptr_t)a->w % 16 == 0) && ((uintptr_t)a->bias % 16 == 0) && ((uintptr_t)a->out % 8 == 0),
           "%s: misaligned tensor", who);
  p.x = (const char*)a->x; p.w = (const bf16_t*)a->w; p.bias = a->bias; p.out = (char*)a->out;
  p.T = a->T; p.H = a->H; p.W = a->W;
  p.To = a->kt == 3 ? sf_pose_out_size(a->T, 3, a->stride_t) : a->T;
  p.Ho = sf_pose_out_size(a->H, 3, a->stride_s);
  p.Wo = sf_pose_out_size(a->W, 3, a->stride_s);
  p.Cout = a->Cout; p.ldw = a->ldw; p.ldo = a->ldo; p.silu = a->silu ? 1 : 0;
  return 0;
}

// x holds p.T frames and out p.To frames: both under the 4 GiB of the kernel's 32-bit offsets
int check_4g(const sf_pose_conv_args* a, const PConvP& p, const char* who) {
  const long xb = (long)p.T * a->H * a->W * a->Cin * 2, ob = (long)p.To * p.Ho * p.Wo * a->ldo * 2;
  SF_CHECK(xb < 0xFFFFFF00L, "%s: input volume of %ld bytes exceeds the 4 GiB the kernel's 32-bit offsets cover", who, xb);
  SF_CHECK(ob < 0xFFFFFF00L, "%s: output volume of %ld bytes exceeds the 4 GiB the kernel's 32-bit offsets cover", who, ob);
  return 0;
}

}  // namespace

extern "C" int sf_pose_conv(const sf_pose_conv_args* a, void* stream) {
  const char* who = "sf_pose_conv";
  PConvP p;
  int nb = 0;
  if (const int rc = conv_setup(a, who, p, nb)) return rc;
  if (const int rc = check_4g(a, p, who)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int key = (a->Cin == 16) * 1000 + a->kt * 100 + a->stride_t * 10 + a->stride_s;
  if (nb == 1) {
    switch (key) {
      case 311: return launch<8, 3, 1, 1, 1>(p, who, s);
      case 1311: return launch<16, 3, 1, 1, 1>(p, who, s);
      case 1312: return launch<16, 3, 1, 2, 1>(p, who, s);
      case 1322: return launch<16, 3, 2, 2, 1>(p, who, s);
      case 111: return launch<8, 1, 1, 1, 1>(p, who, s);
      case 1111: return launch<16, 1, 1, 1, 1>(p, who, s);
      case 1112: return launch<16, 1, 1, 2, 1>(p, who, s);
      default: break;
    }
  } else if (key == 1112) {
    return launch<16, 1, 1, 2, 2>(p, who, s);
  }
  SF_CHECK(false, "sf_pose_conv: no kernel for Cin=%d kt=%d stride (%d, %d) Cout=%d (the pose stacks do not use it)", a->Cin, a->kt, a->stride_t,
           a->stride_s, a->Cout);
}

extern "C" int sf_pose_conv_window(const sf_pose_conv_args* a, const sf_pose_window* win, void* stream) {
  const char* who = "sf_pose_conv_window";
  PConvP p;
  int nb = 0;
  if (const int rc = conv_setup(a, who, p, nb)) return rc;
  SF_CHECK(win != nullptr, "%s: null window", who);
  const int st = a->stride_t;
  const int key = (a->Cin == 16) * 1000 + a->kt * 100 + st * 10 + a->stride_s;
  SF_CHECK(nb == 1 && (key == 311 || key == 1311 || key == 1312 || key == 1322),
           "%s: no kernel for Cin=%d kt=%d stride (%d, %d) Cout=%d (the window mode serves the dwpose stack's 3x3x3 layers)", who, a->Cin, a->kt, st,
           a->stride_s, a->Cout);
  const int lim = 1 << 28;
  SF_CHECK(win->t_end > 0 && win->t_end <= lim && win->x_t0 > -lim && win->x_t0 < lim && win->t_out0 >= 0 && win->t_out0 < lim && win->n_out > 0 &&
               win->n_out < lim,
           "%s: malformed window (x_t0=%d, timeline [0, %d), outputs %d + %d)", who, win->x_t0, win->t_end, win->t_out0, win->n_out);
  const int o_lo = win->t_out0, o_hi = win->t_out0 + win->n_out;        // output frames [o_lo, o_hi)
  // the in-range input frames they read: t*st - 1 .. t*st + 1, clipped to the timeline
  const int need_lo = o_lo * st - 1 < 0 ? 0 : o_lo * st - 1;
  int need_hi = (o_hi - 1) * st + 2;                                    // exclusive
  if (win->closed) {
    SF_CHECK(o_hi <= sf_pose_out_size(win->t_end, 3, st), "%s: output frames [%d, %d) of a closed timeline of %d frames, which gives %d", who, o_lo,
             o_hi, win->t_end, sf_pose_out_size(win->t_end, 3, st));
    if (need_hi > win->t_end) need_hi = win->t_end;                     // frames behind a closed clip are the zero padding
  } else {
    SF_CHECK(need_hi <= win->t_end, "%s: output frames [%d, %d) read input frame %d, but the open timeline ends at %d", who, o_lo, o_hi, need_hi - 1,
             win->t_end);
  }
  SF_CHECK(win->x_t0 <= need_lo && need_hi <= win->x_t0 + a->T,
           "%s: the window holds input frames [%d, %d), output frames [%d, %d) read [%d, %d)", who, win->x_t0, win->x_t0 + a->T, o_lo, o_hi, need_lo,
           need_hi);
  p.To = win->n_out;
  if (const int rc = check_4g(a, p, who)) return rc;
  PWin pw;
  pw.x_t0 = win->x_t0;
  pw.t_lo = win->x_t0 < 0 ? 0 : win->x_t0;
  pw.t_hi = win->x_t0 + a->T < win->t_end ? win->x_t0 + a->T : win->t_end;
  pw.t_out0 = win->t_out0;
  hipStream_t s = (hipStream_t)stream;
  switch (key) {
    case 311: return launch<8, 3, 1, 1, 1>(p, who, s, &pw);
    case 1311: return launch<16, 3, 1, 1, 1>(p, who, s, &pw);
    case 1312: return launch<16, 3, 1, 2, 1>(p, who, s, &pw);
    default: return launch<16, 3, 2, 2, 1>(p, who, s, &pw);
  }
}

extern "C" int sf_pose_prepare(const void* src, int dtype, int hwc, int F, int H, int W, int lead, void* out, void* stream) {
  SF_CHECK(src && out, "sf_pose_prepare: null tensor");
  SF_CHECK(dtype >= SF_POSE_U8 && dtype <= SF_POSE_BF16, "sf_pose_prepare: unknown dtype %d", dtype);
  SF_CHECK(F > 0 && H > 0 && W > 0 && lead >= 0 && lead <= 16, "sf_pose_prepare: F=%d H=%d W=%d lead=%d", F, H, W, lead);
  SF_CHECK(!hwc || F == 1, "sf_pose_prepare: the [H, W, 3] layout holds one image");
  SF_CHECK((uintptr_t)out % 16 == 0, "sf_pose_prepare: misaligned output");
  const long hw = (long)H * W;
  SF_CHECK(hw < (1L << 31), "sf_pose_prepare: frame too large");
  const long n_pos = (long)(F + lead) * hw;
  SF_CHECK(n_pos * 16 < 0xFFFFFF00L, "sf_pose_prepare: prepared volume of %ld bytes exceeds the 4 GiB the convolution's 32-bit offsets cover", n_pos * 16);
  const dim3 grid((unsigned)((n_pos + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  const long plane = (long)F * hw;
  static_assert(SF_POSE_U8 == (int)SF_JPEG_U8 && SF_POSE_F32 == (int)SF_JPEG_F32 && SF_POSE_BF16 == (int)SF_JPEG_BF16, "pixel_dispatch reads sf_pose_dtype");
  return pixel_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return sf_launch<&pose_prepare_kernel<T>>("sf_pose_prepare", grid, dim3(256), 0, s, (const T*)src, (bf16_t*)out, n_pos, (int)hw, plane, hwc, lead);
  });
}
