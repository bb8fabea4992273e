// Implicit-GEMM convolution on channels-last bf16 volumes for gfx950 (MI355X).
//
// Replaces, on the VAE decode path, CausalConv3d (3x3x3, (3,1,1) and 1x1x1: wan/modules/vae.py:17-38),
// the per-frame nn.Conv2d 3x3 of Resample INCLUDING the nearest-neighbour 2x upsampling in front of it
// (vae.py:77-83, :139-141: the 4x larger tensor is never materialised), the bias add, the residual add
// of ResidualBlock (vae.py:221), the channel->frame interleave after the time convolution
// (vae.py:134-137) and the final float / clamp(-1, 1) of decode_to_pixel (utils/wan_wrapper.py:113).
//
//   out[(t,h,w)][n] = bias[n] + sum over taps (dt,dh,dw), ci of
//                     x[t + dt + t_off][(h + dh - kh/2) >> up][(w + dw - kw/2) >> up][ci] * wk[n][tap*Cin + ci]
//
// or, with the strided gathers of the VAE encoder's downsampling (Resample 'downsample2d/3d', vae.py:87-97, :143-160:
// ZeroPad2d((0,1,0,1)) + Conv2d 3x3 stride 2, and the (3,1,1) time convolution with temporal stride 2),
//                     x[st t + dt + t_off][2h + dh][2w + dw][ci]   (spatial stride 2: no left / top padding; taps past
//                                                                   the right / bottom edge read zero)
//
// i.e. a GEMM with M = Tout*H*W output positions, N = Cout, K = taps*Cin whose A operand is GATHERED:
// K is walked in 32-channel slices (Cin % 32 == 0), two slices per 64-deep k-step, every slice lies
// inside one tap, and a lane's 16-byte piece of an A row comes from the tap-shifted position or -- for
// the zero padding in h/w, rows past M and the padding slice of an odd slice count -- from an offset past the
// end of the volume, which the range-checked LDS-DMA (buffer_load ... lds) turns into zeros.  Causality costs nothing here: the input volume holds the two history frames physically in
// front of the new ones (the caller keeps them there), so t + dt never leaves the buffer.
//
// Everything after the gather is the GEMM of gemm_bf16.hip: 128 x (32 NT) output tile per 256-thread
// workgroup, 4 waves as 2x2, 64 x (16 NT) per wave in 16x16x32 bf16 MFMAs, A and W tiles by LDS-DMA
// into two stages, 128-byte LDS rows with the chunk swizzle c ^ ((r>>1)&7) applied on the source side
// and on the ds_read_b128, operands swapped so that a lane owns 4 consecutive output channels.
// NT in {1,2,3,4,6} covers Cout = 3 (head) ... 96, 192, 384, 768 without padding waste.
#include <cstdlib>
#include "sf_common.h"
#include "conv_igemm_core.h"
#include "../../include/sf_hip.h"

namespace {

struct ConvP {
  const bf16_t* x;
  const bf16_t* w;
  const bf16_t* bias;
  bf16_t* out;
  const bf16_t* resid;
  float* out_f32;
  int M, HW, H, W;
  int Hin, Win, up;
  int Hv, Wv;         // bounds of the tap coordinates: the output frame with the upsampling, else the input frame
  int sh, st;         // spatial / temporal input stride (1 or 2)
  int Cin, Cout, cpt, ntaps, khw, kw, ph, pw;
  int t_off, nk, ldw, ldo, ldr, out_frame0, inter_c, Tout;
  int tiles_m, tiles_n;
  unsigned x_bytes;   // size of the input volume the gather may touch (range check of the LDS-DMA)
  // what conv_igemm_core.h asks of its caller: all run-time here
  __device__ __forceinline__ int stride_hw() const { return sh; }
  __device__ __forceinline__ int stride_t() const { return st; }
  __device__ __forceinline__ int pad_h() const { return ph; }
  __device__ __forceinline__ int pad_w() const { return pw; }
  __device__ __forceinline__ int tap_h() const { return Hv; }
  __device__ __forceinline__ int tap_w() const { return Wv; }
  __device__ __forceinline__ int frame_off() const { return t_off; }
  __device__ __forceinline__ bool spatial3x3() const { return khw == 9; }
  __device__ __forceinline__ long resid_row0() const { return (long)out_frame0 * HW; }
  __device__ __forceinline__ void store(int m, int n, const bf16x8& v) const {   // the plain row
    *reinterpret_cast<bf16x8*>(out + ((long)out_frame0 * HW + m) * ldo + n) = v;
  }
};

template <int NT, int EPI>
__global__ __launch_bounds__(igemm::THREADS, 2) void conv_igemm_kernel(ConvP p) {
  constexpr int BN = 32 * NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // XCD-aware bijective remap, then row-tile-major order: consecutive workgroups of one XCD work on
  // neighbouring output positions, whose gathered inputs overlap (taps) and share that XCD's L2
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wg = sf_xcd_remap(bid, nwg);
  const int tm = wg / p.tiles_n, tn = wg - tm * p.tiles_n;
  const int m0 = tm * igemm::BM, n0 = tn * BN;

#include "conv_igemm_mainloop.inc"

  // ---- epilogue: the lane holds out[m][n .. n+3] for (mt, nt); m = mrow + 16 mt, n = ncol + 16 nt
  const int mrow = m0 + wr * 64 + (lane & 15);
  const int ncol = n0 + wc * (16 * NT) + (lane >> 4) * 4;
  if (EPI != SF_CONV_BIAS_CLAMP_F32 && p.inter_c == 0 && (p.Cout & 7) == 0 && (p.ldo & 7) == 0) {
    constexpr bool EPI_BIAS = true, EPI_RESID = EPI == SF_CONV_BIAS_RESID, EPI_RELU = false;
#include "conv_igemm_epilogue.inc"
    return;
  }
  // the direct 8-byte form: the channel -> frame interleave, Cout or ldo not a multiple of 8, the float head
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int m = mrow + mt * 16;
    if (m >= p.M) continue;
    const int t = m / p.HW, hw = m - t * p.HW;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = ncol + nt * 16;
      if (n >= p.Cout) continue;
      float y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = acc[mt][nt][j];
      if (EPI == SF_CONV_BIAS_CLAMP_F32) {
        // Cout is tiny (3): per-element guards, planar float output [Tout][Cout][H][W]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (n + j < p.Cout) {
            const float v = y[j] + (float)p.bias[n + j];
            p.out_f32[((long)t * p.Cout + n + j) * p.HW + hw] = fminf(fmaxf(v, -1.f), 1.f);
          }
        }
        continue;
      }
      const bf16x4 b = *reinterpret_cast<const bf16x4*>(p.bias + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] += (float)b[j];
      // channel -> frame interleave of the time convolution: channels [0,C) are frame 2t, [C,2C) frame 2t+1
      int tf = t, nn = n;
      if (p.inter_c > 0) {
        const int sel = n >= p.inter_c ? 1 : 0;
        tf = 2 * t + sel;
        nn = n - sel * p.inter_c;
      }
      const long row = (long)(p.out_frame0 + tf) * p.HW + hw;
      if (EPI == SF_CONV_BIAS_RESID) {
        const bf16x4 rv = *reinterpret_cast<const bf16x4*>(p.resid + row * p.ldr + nn);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] += (float)rv[j];
      }
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16_t)y[j];
      *reinterpret_cast<bf16x4*>(p.out + row * p.ldo + nn) = o;
    }
  }
}

template <int NT>
int launch_nt(const ConvP& p, int epi, hipStream_t s) {
  constexpr int LDS = igemm::lds_bytes(NT);
  const dim3 grid(p.tiles_m * p.tiles_n), block(igemm::THREADS);
  switch (epi) {   // (LDS is above the 64 KiB an unregistered kernel may use at NT = 6 only)
    case SF_CONV_BIAS: return sf_launch<&conv_igemm_kernel<NT, SF_CONV_BIAS>, LDS>("sf_conv_igemm", grid, block, LDS, s, p);
    case SF_CONV_BIAS_RESID: return sf_launch<&conv_igemm_kernel<NT, SF_CONV_BIAS_RESID>, LDS>("sf_conv_igemm", grid, block, LDS, s, p);
    case SF_CONV_BIAS_CLAMP_F32: return sf_launch<&conv_igemm_kernel<NT, SF_CONV_BIAS_CLAMP_F32>, LDS>("sf_conv_igemm", grid, block, LDS, s, p);
    default: SF_CHECK(false, "sf_conv_igemm: unknown epilogue %d", epi);
  }
}

}  // namespace

extern "C" int sf_conv_pick_nt(int cout) {
  // the per-wave column count (16 NT) that pads Cout least; ties go to the larger tile
  const int cand[5] = {6, 4, 3, 2, 1};
  int best = 1;
  long best_cost = -1;
  for (int i = 0; i < 5; ++i) {
    const int bn = 32 * cand[i];
    const long cost = (long)((cout + bn - 1) / bn) * bn;
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = cand[i]; }
  }
  return best;
}

int sf_conv_halo_launch(const sf_conv_args* a, void* stream);   // conv_halo.hip: 1 = outside its domain

extern "C" int sf_conv_igemm(const sf_conv_args* a, void* stream) {
  SF_CHECK(a != nullptr, "sf_conv_igemm: null args");
  SF_CHECK(a->structure >= SF_CONV_AUTO && a->structure <= SF_CONV_HALO, "sf_conv_igemm: unknown structure %d", a->structure);
  SF_CHECK(a->x && a->w && a->bias, "sf_conv_igemm: null tensor");
  SF_CHECK(!a->norm_out || a->structure != SF_CONV_IGEMM, "sf_conv_igemm: the fused norm output exists in the halo kernel only");
  SF_CHECK(a->structure != SF_CONV_HALO || (a->stride_hw <= 1 && a->stride_t <= 1), "sf_conv_igemm: the halo structure takes no strided input");
  SF_CHECK(a->Tout > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0, "sf_conv_igemm: empty problem");
  SF_CHECK(a->Cin % 32 == 0, "sf_conv_igemm: Cin=%d must be a multiple of 32 (pad the channels)", a->Cin);
  SF_CHECK((a->kh == 3 && a->kw == 3) || (a->kh == 1 && a->kw == 1), "sf_conv_igemm: spatial taps must be 3x3 or 1x1");
  SF_CHECK(a->kt == 1 || a->kt == 3, "sf_conv_igemm: kt must be 1 or 3");
  SF_CHECK(a->upsample == 0 || a->upsample == 1, "sf_conv_igemm: upsample must be 0 or 1");
  SF_CHECK(a->stride_hw >= 0 && a->stride_hw <= 2 && a->stride_t >= 0 && a->stride_t <= 2, "sf_conv_igemm: strides %d / %d (0 or 1: none, 2: stride 2)",
           a->stride_hw, a->stride_t);
  const int sh = a->stride_hw == 2 ? 2 : 1, st = a->stride_t == 2 ? 2 : 1;
  SF_CHECK(sh == 1 || (!a->upsample && a->kh == 3 && a->kw == 3), "sf_conv_igemm: spatial stride 2 is a 3x3 convolution without upsampling");
  if (sh == 2) {   // ZeroPad2d((0,1,0,1)) + stride 2: H = floor(Hin / 2)
    SF_CHECK(a->Hin / 2 == a->H && a->Win / 2 == a->W, "sf_conv_igemm: stride-2 input size %dx%d does not match output %dx%d", a->Hin, a->Win, a->H, a->W);
  } else {
    SF_CHECK(a->Hin == (a->upsample ? a->H / 2 : a->H) && a->Win == (a->upsample ? a->W / 2 : a->W) &&
             (!a->upsample || (a->H % 2 == 0 && a->W % 2 == 0)), "sf_conv_igemm: input size %dx%d does not match output %dx%d", a->Hin, a->Win, a->H, a->W);
  }
  const int taps = a->kt * a->kh * a->kw;
  const int slices = taps * (a->Cin / 32);
  const int nk = (slices + 1) / 2;
  SF_CHECK(a->ldw >= nk * 64 && a->ldw % 8 == 0, "sf_conv_igemm: weight row stride %d < padded K %d", a->ldw, nk * 64);
  SF_CHECK((long)a->Tout * a->H * a->W < (1L << 31), "sf_conv_igemm: too many output positions");
  SF_CHECK(a->t_in_offset >= 0, "sf_conv_igemm: negative input frame offset");
  SF_CHECK(((uintptr_t)a->x % 16 == 0) && ((uintptr_t)a->w % 16 == 0) && ((uintptr_t)a->bias % 8 == 0), "sf_conv_igemm: misaligned tensor");
  if (a->epilogue == SF_CONV_BIAS_CLAMP_F32) {
    SF_CHECK(a->out_f32 != nullptr && a->interleave_c == 0, "sf_conv_igemm: float epilogue needs out_f32 and no interleave");
  } else {
    SF_CHECK((a->out != nullptr || a->norm_out != nullptr) && a->Cout % 4 == 0, "sf_conv_igemm: bf16 output needs out (or norm_out) and Cout %% 4 == 0");
    SF_CHECK(!a->out || (a->ldo % 4 == 0 && (uintptr_t)a->out % 8 == 0), "sf_conv_igemm: misaligned output / ldo %% 4 != 0");
    SF_CHECK(!a->norm_out || ((uintptr_t)a->norm_out % 16 == 0 && (uintptr_t)a->norm_gamma % 16 == 0), "sf_conv_igemm: misaligned norm output");
    SF_CHECK(a->interleave_c == 0 || (a->interleave_c * 2 == a->Cout && a->interleave_c % 4 == 0), "sf_conv_igemm: interleave_c must be Cout/2");
    SF_CHECK(!a->out || a->ldo >= (a->interleave_c ? a->interleave_c : a->Cout), "sf_conv_igemm: ldo too small");
    if (a->epilogue == SF_CONV_BIAS_RESID)
      SF_CHECK(a->resid != nullptr && a->ldr % 4 == 0 && a->ldr >= a->Cout && a->interleave_c == 0, "sf_conv_igemm: residual epilogue needs resid/ldr");
  }
  if (a->structure != SF_CONV_IGEMM) {
    // 3 x 3 convolutions with 96 k / 192 k output channels: the halo-tile kernel (the A operand staged once per
    // (channel slice, frame) instead of once per tap), conv_halo.hip
    const int rc = sf_conv_halo_launch(a, stream);
    if (rc <= 0) return rc;   // launched, or the launch failed
    SF_CHECK(a->structure == SF_CONV_AUTO && !a->norm_out, "sf_conv_igemm: the halo structure needs 3x3 spatial taps, "
             "Cout %% 96 == 0 (a fused norm output: Cout 96 or 192, norm_ld %% 8 == 0), H, W >= 16, ldo %% 8 == 0, a bf16 bias / bias + residual "
             "epilogue and no interleave");
  }
  ConvP p;
  p.x = (const bf16_t*)a->x; p.w = (const bf16_t*)a->w; p.bias = (const bf16_t*)a->bias;
  p.out = (bf16_t*)a->out; p.resid = (const bf16_t*)a->resid; p.out_f32 = a->out_f32;
  p.HW = a->H * a->W; p.M = a->Tout * p.HW; p.H = a->H; p.W = a->W; p.Tout = a->Tout;
  p.Hin = a->Hin; p.Win = a->Win; p.up = a->upsample;
  p.Hv = a->upsample ? a->H : a->Hin; p.Wv = a->upsample ? a->W : a->Win; p.sh = sh; p.st = st;
  p.Cin = a->Cin; p.Cout = a->Cout; p.cpt = a->Cin / 32; p.ntaps = taps; p.khw = a->kh * a->kw; p.kw = a->kw;
  p.ph = sh == 2 ? 0 : a->kh / 2; p.pw = sh == 2 ? 0 : a->kw / 2;
  p.t_off = a->t_in_offset; p.nk = nk; p.ldw = a->ldw; p.ldo = a->ldo; p.ldr = a->ldr;
  p.out_frame0 = a->out_frame_offset; p.inter_c = a->interleave_c;
  {   // frames [0, t_in_offset + st (Tout - 1) + kt) of the input volume can be gathered from
    const long xb = (long)(a->t_in_offset + (long)st * (a->Tout - 1) + a->kt) * a->Hin * a->Win * a->Cin * 2;
    SF_CHECK(xb < 0xFFFFFF00L, "sf_conv_igemm: input volume of %ld bytes exceeds the 4 GiB the gather's 32-bit offsets cover", xb);
    p.x_bytes = (unsigned)xb;
  }
  const int nt = sf_conv_pick_nt(a->Cout);
  p.tiles_m = (p.M + igemm::BM - 1) / igemm::BM;
  p.tiles_n = (a->Cout + 32 * nt - 1) / (32 * nt);
  hipStream_t s = (hipStream_t)stream;
  switch (nt) {
    case 1: return launch_nt<1>(p, a->epilogue, s);
    case 2: return launch_nt<2>(p, a->epilogue, s);
    case 3: return launch_nt<3>(p, a->epilogue, s);
    case 4: return launch_nt<4>(p, a->epilogue, s);
    default: return launch_nt<6>(p, a->epilogue, s);
  }
}
