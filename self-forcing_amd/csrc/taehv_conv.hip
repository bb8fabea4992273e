// The 3x3 convolution of the TAEHV tiny decoder on channels-last bf16 volumes for gfx950 (MI355X).
//
// Replaces, on the TAEHV decode path (demo_utils/taehv.py), every nn.Conv2d 3x3 of the decoder (:16-17, :181-190)
// together with what surrounds it: the torch.cat([x, past], 1) in front of a MemBlock's first convolution (:33-34),
// the nn.ReLU after a convolution (:28-31, :182, :189), the residual add + ReLU that end a MemBlock (:34), the
// nn.Upsample(scale_factor=2) in front of a stage's exit convolution (:183-188; the 4x larger tensor is never
// materialised), the TGrow 1x1 convolution and its channel -> frame re-read (:48-57; folded into the exit convolution's
// weights by the host, so only the re-read remains, as the epilogue's frame interleave), and the `* 2 - 1` of the demo
// wrapper with the clamp of decode_to_pixel (demo.py:84-89, utils/wan_wrapper.py:113) on the 64 -> 3 head.
//
//   out[(t,h,w)][n] = epi( bias[n] + sum over taps (dt,dh,dw), ci of
//                          x[t + dt][(h + dh - 1) >> up][(w + dw - 1) >> up][ci] * wk[n][((dt*3 + dh)*3 + dw)*Cin + ci] )
//
// conv(cat[x_t, x_{t-1}]) is a causal convolution with kt = 2 temporal taps over a volume that holds the previous frame
// physically in front of the new ones: tap dt = 0 reads frame t - 1 with weight[:, C:], tap dt = 1 frame t with
// weight[:, :C].  Nothing is concatenated, and a group of frames is one launch.
//
// The structure is conv_igemm.hip's -- GEMM with M = Tout*H*W, N = Cout, K = kt*9*Cin, the A tile GATHERED by the
// range-checked LDS-DMA (zero padding = an offset past the end of the volume), 128 x (32 NT) output tile per 256-thread
// workgroup, 4 waves as 2x2 in 16x16x32 bf16 MFMAs, two LDS stages, 128-byte rows with the chunk swizzle on the source
// side -- and so is the code: the gather, the main loop and the through-LDS epilogue are conv_igemm_core.h's.  This file
// adds to the core: kt in {1, 2}, always 3x3 and unstrided as compile-time geometry (the tap arithmetic folds to a shorter
// form), NT in {4, 2, 1} for Cout = 256 / 128, 64 and 3 without padding waste, the ReLU epilogues, the interleave through
// the coalesced LDS write-back (the 64-channel volumes at 240x416 and 480x832 hold most of the decoder's bytes) and the
// float heads (the decoder's 2 y - 1 with its clamp; the encoder's 64 -> 16 latents, y + bias as they are).
#include <cstdlib>
#include "conv_igemm_core.h"
#include "../../include/sf_hip.h"

namespace {

struct TConvP {
  const bf16_t* x;
  const bf16_t* w;
  const bf16_t* bias;
  bf16_t* out;
  const bf16_t* resid;
  float* out_f32;
  int M, HW, H, W;
  int Hin, Win, up;
  int Cin, Cout, cpt, ntaps;
  int nk, ldw, ldo, ldr, tgrow, inter_c, clamp;
  int tiles_m, tiles_n;
  unsigned x_bytes;   // size of the input volume the gather may touch (range check of the LDS-DMA)
  // what conv_igemm_core.h asks of its caller: always 3x3, unstrided, padded by 1, no frame offset -- compile-time here
  __device__ __forceinline__ static constexpr int stride_hw() { return 1; }
  __device__ __forceinline__ static constexpr int stride_t() { return 1; }
  __device__ __forceinline__ static constexpr int pad_h() { return 1; }
  __device__ __forceinline__ static constexpr int pad_w() { return 1; }
  __device__ __forceinline__ int tap_h() const { return H; }
  __device__ __forceinline__ int tap_w() const { return W; }
  __device__ __forceinline__ static constexpr int frame_off() { return 0; }
  __device__ __forceinline__ static constexpr bool spatial3x3() { return true; }
  __device__ __forceinline__ static constexpr long resid_row0() { return 0; }
  // TGrow's re-read: channels [s C', (s+1) C') of input frame t are output frame tgrow t + s (tgrow 1: s = 0).  With the
  // frame interleave a row's two halves go to two frames, each half one contiguous run of inter_c channels.
  __device__ __forceinline__ void store(int m, int n, const bf16x8& v) const {
    const int t = m / HW, hw = m - t * HW;
    const int sel = n >= inter_c ? 1 : 0;
    const long orow = (long)(tgrow * t + sel) * HW + hw;
    *reinterpret_cast<bf16x8*>(out + orow * ldo + (n - sel * inter_c)) = v;
  }
};

template <int NT, int EPI>
__global__ __launch_bounds__(igemm::THREADS, 2) void taehv_conv_kernel(TConvP p) {
  constexpr int BN = 32 * NT;
  constexpr bool F32_OUT = EPI == SF_TAEHV_HEAD_F32 || EPI == SF_TAEHV_LATENT_F32;
  constexpr bool HAS_BIAS = EPI == SF_TAEHV_BIAS_RELU || EPI == SF_TAEHV_BIAS_RESID_RELU || F32_OUT;
  constexpr bool RELU = EPI != SF_TAEHV_PLAIN && !F32_OUT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // XCD-aware bijective remap, then row-tile-major order: consecutive workgroups of one XCD work on neighbouring
  // output positions, whose gathered inputs overlap (taps) and share that XCD's L2
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wg = sf_xcd_remap(bid, nwg);
  const int tm = wg / p.tiles_n, tn = wg - tm * p.tiles_n;
  const int m0 = tm * igemm::BM, n0 = tn * BN;

#include "conv_igemm_mainloop.inc"

  // ---- epilogue: the lane holds y[m][n .. n+3] for (mt, nt); m = m0 + wr*64 + 16 mt + (lane & 15), n = n0 + wc*16NT + 16 nt + 4 (lane >> 4)
  if (F32_OUT) {
    // Cout is tiny (3, or the encoder's 16): per-element guards, planar float output [Tout][Cout][H][W] = 2 (y + bias) - 1
    // (the encoder's latents: y + bias); 16 lanes write 16 consecutive positions of one plane
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = m0 + wr * 64 + mt * 16 + (lane & 15);
      if (m >= p.M) continue;
      const int t = m / p.HW, hw = m - t * p.HW;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + wc * (16 * NT) + nt * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (n + j < p.Cout) {
            float v = acc[mt][nt][j] + (float)p.bias[n + j];
            if (EPI == SF_TAEHV_HEAD_F32) {
              v = 2.0f * v - 1.0f;
              if (p.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
            }
            p.out_f32[((long)t * p.Cout + n + j) * p.HW + hw] = v;
          }
        }
      }
    }
    return;
  }
  constexpr bool EPI_BIAS = HAS_BIAS, EPI_RESID = EPI == SF_TAEHV_BIAS_RESID_RELU, EPI_RELU = RELU;
#include "conv_igemm_epilogue.inc"
}

template <int NT, int EPI>
int launch_epi(const TConvP& p, hipStream_t s) {
  constexpr int LDS = igemm::lds_bytes(NT);
  static_assert(LDS <= 64 * 1024, "the tiles of this kernel fit the default dynamic-LDS limit");
  static_assert(igemm::BM * igemm::out_row_bytes(NT) <= LDS, "the epilogue's output tile fits the stages");
  return sf_launch<&taehv_conv_kernel<NT, EPI>>("sf_taehv_conv", dim3(p.tiles_m * p.tiles_n), dim3(igemm::THREADS), LDS, s, p);
}

template <int NT>
int launch_nt(const TConvP& p, int epi, hipStream_t s) {
  switch (epi) {
    case SF_TAEHV_BIAS_RELU: return launch_epi<NT, SF_TAEHV_BIAS_RELU>(p, s);
    case SF_TAEHV_BIAS_RESID_RELU: return launch_epi<NT, SF_TAEHV_BIAS_RESID_RELU>(p, s);
    case SF_TAEHV_PLAIN: return launch_epi<NT, SF_TAEHV_PLAIN>(p, s);
    case SF_TAEHV_RELU: return launch_epi<NT, SF_TAEHV_RELU>(p, s);
    case SF_TAEHV_HEAD_F32: return launch_epi<NT, SF_TAEHV_HEAD_F32>(p, s);
    case SF_TAEHV_LATENT_F32: return launch_epi<NT, SF_TAEHV_LATENT_F32>(p, s);
    default: SF_CHECK(false, "sf_taehv_conv: unknown epilogue %d", epi);
  }
}

}  // namespace

extern "C" int sf_taehv_pick_nt(int cout) {
  // the per-wave column count (16 NT): 128-wide tiles for Cout = 256 / 128, 64-wide for 64, 32-wide for the head
  return cout % 128 == 0 ? 4 : cout % 64 == 0 ? 2 : 1;
}

extern "C" int sf_taehv_conv(const sf_taehv_conv_args* a, void* stream) {
  SF_CHECK(a != nullptr, "sf_taehv_conv: null args");
  SF_CHECK(a->x && a->w, "sf_taehv_conv: null tensor");
  SF_CHECK(a->epilogue >= SF_TAEHV_BIAS_RELU && a->epilogue <= SF_TAEHV_LATENT_F32, "sf_taehv_conv: unknown epilogue %d", a->epilogue);
  SF_CHECK(a->Tout > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0, "sf_taehv_conv: empty problem");
  SF_CHECK(a->Cin % 32 == 0, "sf_taehv_conv: Cin=%d must be a multiple of 32 (pad the channels)", a->Cin);
  SF_CHECK(a->kt == 1 || a->kt == 2, "sf_taehv_conv: kt must be 1 or 2, got %d", a->kt);
  SF_CHECK(a->upsample == 0 || a->upsample == 1, "sf_taehv_conv: upsample must be 0 or 1");
  SF_CHECK(!a->upsample || (a->H % 2 == 0 && a->W % 2 == 0), "sf_taehv_conv: an upsampled output %dx%d must be even", a->H, a->W);
  const bool f32_out = a->epilogue == SF_TAEHV_HEAD_F32 || a->epilogue == SF_TAEHV_LATENT_F32;
  const bool has_bias = a->epilogue == SF_TAEHV_BIAS_RELU || a->epilogue == SF_TAEHV_BIAS_RESID_RELU || f32_out;
  SF_CHECK(!has_bias || a->bias, "sf_taehv_conv: epilogue %d needs a bias", a->epilogue);
  const int slices = a->kt * 9 * (a->Cin / 32);
  const int nk = (slices + 1) / 2;
  SF_CHECK(a->ldw >= nk * 64 && a->ldw % 8 == 0, "sf_taehv_conv: weight row stride %d < padded K %d", a->ldw, nk * 64);
  SF_CHECK((long)a->Tout * a->H * a->W < (1L << 31), "sf_taehv_conv: too many output positions");
  SF_CHECK(((uintptr_t)a->x % 16 == 0) && ((uintptr_t)a->w % 16 == 0) && ((uintptr_t)a->bias % 8 == 0), "sf_taehv_conv: misaligned tensor");
  const int tgrow = a->tgrow <= 1 ? 1 : a->tgrow;
  SF_CHECK(tgrow <= 2, "sf_taehv_conv: tgrow must be 1 or 2, got %d", a->tgrow);
  if (f32_out) {
    SF_CHECK(a->out_f32 != nullptr && tgrow == 1 && a->Cout <= 32, "sf_taehv_conv: the float head needs out_f32, no tgrow and Cout <= 32");
  } else {
    SF_CHECK(a->out != nullptr && a->Cout % 8 == 0, "sf_taehv_conv: bf16 output needs out and Cout %% 8 == 0");
    SF_CHECK(a->ldo % 8 == 0 && (uintptr_t)a->out % 16 == 0, "sf_taehv_conv: misaligned output / ldo %% 8 != 0");
    SF_CHECK(a->Cout % (8 * tgrow) == 0 && a->ldo >= a->Cout / tgrow, "sf_taehv_conv: ldo %d too small for %d channels per frame", a->ldo, a->Cout / tgrow);
    SF_CHECK(tgrow == 1 || a->epilogue == SF_TAEHV_PLAIN || a->epilogue == SF_TAEHV_RELU, "sf_taehv_conv: tgrow goes with the bias-free epilogues");
    if (a->epilogue == SF_TAEHV_BIAS_RESID_RELU)
      SF_CHECK(a->resid != nullptr && a->ldr % 4 == 0 && a->ldr >= a->Cout && (uintptr_t)a->resid % 8 == 0, "sf_taehv_conv: residual epilogue needs resid/ldr");
  }
  TConvP p;
  p.x = (const bf16_t*)a->x; p.w = (const bf16_t*)a->w; p.bias = (const bf16_t*)a->bias;
  p.out = (bf16_t*)a->out; p.resid = (const bf16_t*)a->resid; p.out_f32 = a->out_f32;
  p.HW = a->H * a->W; p.M = a->Tout * p.HW; p.H = a->H; p.W = a->W;
  p.up = a->upsample; p.Hin = a->upsample ? a->H / 2 : a->H; p.Win = a->upsample ? a->W / 2 : a->W;
  p.Cin = a->Cin; p.Cout = a->Cout; p.cpt = a->Cin / 32; p.ntaps = a->kt * 9;
  p.nk = nk; p.ldw = a->ldw; p.ldo = a->ldo; p.ldr = a->ldr; p.tgrow = tgrow; p.inter_c = a->Cout / tgrow; p.clamp = a->clamp;
  {   // frames [0, Tout - 1 + kt) of the input volume can be gathered from
    const long xb = (long)(a->Tout - 1 + a->kt) * p.Hin * p.Win * a->Cin * 2;
    SF_CHECK(xb < 0xFFFFFF00L, "sf_taehv_conv: input volume of %ld bytes exceeds the 4 GiB the gather's 32-bit offsets cover", xb);
    p.x_bytes = (unsigned)xb;
  }
  const int nt = sf_taehv_pick_nt(a->Cout);
  p.tiles_m = (p.M + igemm::BM - 1) / igemm::BM;
  p.tiles_n = (a->Cout + 32 * nt - 1) / (32 * nt);
  hipStream_t s = (hipStream_t)stream;
  switch (nt) {
    case 4: return launch_nt<4>(p, a->epilogue, s);
    case 2: return launch_nt<2>(p, a->epilogue, s);
    default: return launch_nt<1>(p, a->epilogue, s);
  }
}
