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
// side -- but its own kernel: kt in {1, 2}, always 3x3 and unstrided (the tap arithmetic is shorter), NT in {4, 2, 1}
// for Cout = 256 / 128, 64 and 3 without padding waste, the ReLU epilogues, the interleave through the coalesced LDS
// write-back (the 64-channel volumes at 240x416 and 480x832 hold most of the decoder's bytes) and the float head.
#include <cstdlib>
#include "lds_dma.h"
#include "../../include/sf_hip.h"

namespace {

constexpr int TBM = 128, TBK = 64;
constexpr int TCONV_THREADS = 256;
constexpr int TA_TILE_BYTES = TBM * TBK * 2;   // 16 KiB

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
};

template <int NT, int EPI>
__global__ __launch_bounds__(TCONV_THREADS, 2) void taehv_conv_kernel(TConvP p) {
  constexpr int BN = 32 * NT;
  constexpr int W_TILE_BYTES = BN * TBK * 2;
  constexpr int STAGE = TA_TILE_BYTES + W_TILE_BYTES;
  constexpr bool HAS_BIAS = EPI == SF_TAEHV_BIAS_RELU || EPI == SF_TAEHV_BIAS_RESID_RELU || EPI == SF_TAEHV_HEAD_F32;
  constexpr bool RELU = EPI != SF_TAEHV_PLAIN && EPI != SF_TAEHV_HEAD_F32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // XCD-aware bijective remap, then row-tile-major order: consecutive workgroups of one XCD work on neighbouring
  // output positions, whose gathered inputs overlap (taps) and share that XCD's L2
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wg = sf_xcd_remap(bid, nwg);
  const int tm = wg / p.tiles_n, tn = wg - tm * p.tiles_n;
  const int m0 = tm * TBM, n0 = tn * BN;

  // ---- the four A pieces of this lane: row r of the tile, 16-byte chunk c of the 128-byte LDS row (chunks 0-3 hold the
  // first 32-channel slice of the k-step, 4-7 the second).  What does not depend on the tap is computed once: the byte
  // offset of the piece at tap (0, 0, 0) and a 9-bit mask of the spatial taps inside the image.  An invalid piece (zero
  // padding, rows past M, the padding slice of an odd slice count) gets an out-of-range offset: the range-checked
  // buffer load writes zeros to LDS.
  unsigned abase[4], vmask[4], parh[4], parw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + (lane >> 3);
    const int c = lds_swizzle(r, lane & 7);
    const int m = m0 + r;
    const bool valid = m < p.M;
    const int mm = min(m, p.M - 1);
    const int t = mm / p.HW, hw = mm - t * p.HW;
    const int h = hw / p.W;
    const int hh0 = h - 1, ww0 = (hw - h * p.W) - 1;
    abase[i] = (unsigned)(((((long)t * p.Hin + (hh0 >> p.up)) * p.Win + (ww0 >> p.up)) * p.Cin + (c & 3) * 8) * 2);
    unsigned vm = 0;
    for (int dh = 0; dh < 3; ++dh)
      for (int dw = 0; dw < 3; ++dw)
        if (valid && (unsigned)(hh0 + dh) < (unsigned)p.H && (unsigned)(ww0 + dw) < (unsigned)p.W) vm |= 1u << (dh * 3 + dw);
    vmask[i] = vm;
    parh[i] = (unsigned)hh0 & 1u;
    parw[i] = (unsigned)ww0 & 1u;
  }
  // piece i lies in slice ((lane >> 2) & 1) ^ (i & 1) of the k-step (from the chunk swizzle above)
  const bool lane_hi = ((lane >> 2) & 1) != 0;
  const bf16_t* w_src[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int r = (wave * NT + j) * 8 + (lane >> 3);
    const int c = lds_swizzle(r, lane & 7);
    const int n = min(n0 + r, p.Cout - 1);
    w_src[j] = p.w + (long)n * p.ldw + c * 8;
  }
  const u32x4 x_srd = lds_dma_srd(p.x, p.x_bytes);
  const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) char*)smem;

  // slice cursor of the NEXT stage to issue: slice = (tap, cc), cc counting 32-channel groups
  int tap = 0, cc = 0;
  const unsigned rowB = (unsigned)(p.Win * p.Cin * 2), colB = (unsigned)(p.Cin * 2), frameB = (unsigned)(p.Hin * p.Win * p.Cin * 2);
  // byte offsets of this lane's four A pieces of the stage the cursor points at; advances the cursor
  auto gather_offsets = [&](unsigned (&voff)[4]) __attribute__((always_inline)) {
    int tap1 = tap, cc1 = cc + 1;
    if (cc1 >= p.cpt) { cc1 -= p.cpt; ++tap1; }
    // tap -> (dt, dh, dw), tap < 32
    const int dt0 = (tap * 57) >> 9, r0 = tap - 9 * dt0, dh0 = (r0 * 11) >> 5, dw0 = r0 - 3 * dh0;
    const int dt1 = (tap1 * 57) >> 9, r1 = tap1 - 9 * dt1, dh1 = (r1 * 11) >> 5, dw1 = r1 - 3 * dh1;
    const unsigned sh0 = tap < p.ntaps ? (unsigned)r0 : 31u, sh1 = tap1 < p.ntaps ? (unsigned)r1 : 31u;
    const unsigned base0 = (unsigned)dt0 * frameB + (unsigned)cc * 64u, base1 = (unsigned)dt1 * frameB + (unsigned)cc1 * 64u;
    // the lane's two slices: pieces 0, 2 use slice `lane_hi`, pieces 1, 3 the other one
    const unsigned shA = lane_hi ? sh1 : sh0, shB = lane_hi ? sh0 : sh1;
    if (p.up == 0) {
      const unsigned d0 = base0 + (unsigned)dh0 * rowB + (unsigned)dw0 * colB, d1 = base1 + (unsigned)dh1 * rowB + (unsigned)dw1 * colB;
      const unsigned dA = lane_hi ? d1 : d0, dB = lane_hi ? d0 : d1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned bad = ((vmask[i] >> ((i & 1) ? shB : shA)) & 1u) - 1u;      // 0 if the tap is inside, ~0 if not
        voff[i] = (abase[i] + ((i & 1) ? dB : dA)) | (bad & 0xFFFFFFF0u);          // (no select: keeps the code branch-free)
      }
    } else {   // fused nearest 2x upsample: the input row / column of a tap depends on the parity of the output position
      const unsigned tA = lane_hi ? base1 : base0, tB = lane_hi ? base0 : base1;
      const unsigned dhA = lane_hi ? dh1 : dh0, dhB = lane_hi ? dh0 : dh1, dwA = lane_hi ? dw1 : dw0, dwB = lane_hi ? dw0 : dw1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned bad = ((vmask[i] >> ((i & 1) ? shB : shA)) & 1u) - 1u;
        const unsigned rdh = (((i & 1) ? dhB : dhA) + parh[i]) >> 1, rdw = (((i & 1) ? dwB : dwA) + parw[i]) >> 1;
        voff[i] = (abase[i] + ((i & 1) ? tB : tA) + rdh * rowB + rdw * colB) | (bad & 0xFFFFFFF0u);
      }
    }
    cc += 2;                                   // advance the cursor by two slices
    if (cc >= p.cpt) { cc -= p.cpt; ++tap; }
    if (cc >= p.cpt) { cc -= p.cpt; ++tap; }
  };

  // ---- fragment read addresses
  const int wr = wave >> 1, wc = wave & 1;
  const int i16 = lane & 15, kq = lane >> 4;
  const int swz = (i16 >> 1) & 7;
  const int x_row_off = (wr * 64 + i16) * 128;                              // + t*2048
  const int w_row_off = TA_TILE_BYTES + (wc * (16 * NT) + i16) * 128;      // + nt*2048
  const int coff0 = ((0 + kq) ^ swz) << 4;
  const int coff1 = ((4 + kq) ^ swz) << 4;

  f32x4 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  unsigned voff[4];                         // offsets of the stage that the NEXT k-step requests
  {   // prologue: stage 0 requested, the offsets of stage 1 computed
    gather_offsets(voff);
    const unsigned abase_lds = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(wave * 4096));
#pragma unroll
    for (int i = 0; i < 4; ++i) lds_dma16_checked(x_srd, voff[i], abase_lds + i * 1024);
    char* wbase = smem + TA_TILE_BYTES + wave * (NT * 1024);
#pragma unroll
    for (int j = 0; j < NT; ++j) glds16(w_src[j], wbase + j * 1024);
    if (p.nk > 1) {
      gather_offsets(voff);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) voff[i] = 0xFFFFFFF0u;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int kt = 0; kt < p.nk; ++kt) {
    const int cur = kt & 1;
    const char* buf = smem + cur * STAGE;
    // The k-step as 4 + NT pinned slices of {MFMAs of the first 32-deep sub-step, one fragment read of the second, ONE
    // LDS-DMA request of the next stage}, then the second sub-step's MFMAs, under which the gather offsets of the stage
    // after next are computed.  The last k-step re-requests its own W pieces and all-invalid A pieces into the idle
    // buffer so that the body stays branch-free.
    const unsigned abase_lds = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)((cur ^ 1) * STAGE + wave * 4096));
    char* wbase = smem + (cur ^ 1) * STAGE + TA_TILE_BYTES + wave * (NT * 1024);
    const int kn = min(kt + 1, p.nk - 1) * TBK;
    bf16x8 xf0[4], xf1[4], wf0[NT], wf1[NT];
#pragma unroll
    for (int t = 0; t < 4; ++t) xf0[t] = *reinterpret_cast<const bf16x8*>(buf + x_row_off + t * 2048 + coff0);
#pragma unroll
    for (int t = 0; t < NT; ++t) wf0[t] = *reinterpret_cast<const bf16x8*>(buf + w_row_off + t * 2048 + coff0);
    __builtin_amdgcn_sched_barrier(0);
    constexpr int NS = 4 + NT;               // slices
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
#pragma unroll
      for (int q = (4 * NT * sl) / NS; q < (4 * NT * (sl + 1)) / NS; ++q) {
        const int mt = q / NT, nt = q - mt * NT;
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0[nt], xf0[mt], acc[mt][nt], 0, 0, 0);
      }
      if (sl < 4) {
        xf1[sl] = *reinterpret_cast<const bf16x8*>(buf + x_row_off + sl * 2048 + coff1);
        lds_dma16_checked(x_srd, voff[sl], abase_lds + sl * 1024);
      } else {
        wf1[sl - 4] = *reinterpret_cast<const bf16x8*>(buf + w_row_off + (sl - 4) * 2048 + coff1);
        glds16(w_src[sl - 4] + kn, wbase + (sl - 4) * 1024);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kt + 2 < p.nk) {
      gather_offsets(voff);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) voff[i] = 0xFFFFFFF0u;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[nt], xf1[mt], acc[mt][nt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // drains the in-flight LDS-DMA (vmcnt(0)) and orders the stage swap
  }

  // ---- epilogue: the lane holds y[m][n .. n+3] for (mt, nt); m = m0 + wr*64 + 16 mt + (lane & 15), n = n0 + wc*16NT + 16 nt + 4 (lane >> 4)
  if (EPI == SF_TAEHV_HEAD_F32) {
    // Cout is tiny (3): per-element guards, planar float output [Tout][Cout][H][W] = 2 (y + bias) - 1; 16 lanes write 16
    // consecutive positions of one plane
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
            float v = 2.0f * (acc[mt][nt][j] + (float)p.bias[n + j]) - 1.0f;
            if (p.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
            p.out_f32[((long)t * p.Cout + n + j) * p.HW + hw] = v;
          }
        }
      }
    }
    return;
  }
  // Through LDS: the 128 x BN tile is assembled as bf16 rows (padded by 16 B against bank conflicts) and written back
  // in 16-byte pieces along the rows.  With the frame interleave a row's two halves go to two frames, each half one
  // contiguous run of inter_c channels.
  constexpr int RBP = 64 * NT + 16;    // padded row bytes
  char* obuf = smem;                   // (the k-loop's last __syncthreads has released the stages)
  int ncol[NT];
  bf16x4 bias_v[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    ncol[nt] = min(n0 + wc * (16 * NT) + nt * 16 + (lane >> 4) * 4, p.Cout - 4);
    if (HAS_BIAS) bias_v[nt] = *reinterpret_cast<const bf16x4*>(p.bias + ncol[nt]);
  }
  bf16x4 rv[4][NT];
  if (EPI == SF_TAEHV_BIAS_RESID_RELU) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const long m = min(m0 + wr * 64 + mt * 16 + (lane & 15), p.M - 1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) rv[mt][nt] = *reinterpret_cast<const bf16x4*>(p.resid + m * p.ldr + ncol[nt]);
    }
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int row = wr * 64 + mt * 16 + (lane & 15);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = wc * (16 * NT) + nt * 16 + (lane >> 4) * 4;
      float y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = acc[mt][nt][j];
      if (HAS_BIAS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] += (float)bias_v[nt][j];
      }
      if (EPI == SF_TAEHV_BIAS_RESID_RELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] += (float)rv[mt][nt][j];
      }
      if (RELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = fmaxf(y[j], 0.f);
      }
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16_t)y[j];
      *reinterpret_cast<bf16x4*>(obuf + row * RBP + col * 2) = o;
    }
  }
  __syncthreads();
  constexpr int CPR = 4 * NT;          // 16-byte chunks per row
#pragma unroll
  for (int i = 0; i < (TBM * CPR) / TCONV_THREADS; ++i) {
    const int id = i * TCONV_THREADS + tid;
    const int row = id / CPR, ch = id - row * CPR;
    const int m = m0 + row, n = n0 + ch * 8;
    if (m < p.M && n < p.Cout) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(obuf + row * RBP + ch * 16);
      // TGrow's re-read: channels [s C', (s+1) C') of input frame t are output frame tgrow t + s (tgrow 1: s = 0)
      const int t = m / p.HW, hw = m - t * p.HW;
      const int sel = n >= p.inter_c ? 1 : 0;
      const long orow = (long)(p.tgrow * t + sel) * p.HW + hw;
      *reinterpret_cast<bf16x8*>(p.out + orow * p.ldo + (n - sel * p.inter_c)) = v;
    }
  }
}

template <int NT, int EPI>
int launch_epi(const TConvP& p, hipStream_t s) {
  constexpr int LDS = 2 * (TA_TILE_BYTES + 32 * NT * TBK * 2);
  static_assert(LDS <= 64 * 1024, "the tiles of this kernel fit the default dynamic-LDS limit");
  static_assert(TBM * (64 * NT + 16) <= LDS, "the epilogue's output tile fits the stages");
  hipLaunchKernelGGL((taehv_conv_kernel<NT, EPI>), dim3(p.tiles_m * p.tiles_n), dim3(TCONV_THREADS), LDS, s, p);
  return 0;
}

template <int NT>
int launch_nt(const TConvP& p, int epi, hipStream_t s) {
  switch (epi) {
    case SF_TAEHV_BIAS_RELU: return launch_epi<NT, SF_TAEHV_BIAS_RELU>(p, s);
    case SF_TAEHV_BIAS_RESID_RELU: return launch_epi<NT, SF_TAEHV_BIAS_RESID_RELU>(p, s);
    case SF_TAEHV_PLAIN: return launch_epi<NT, SF_TAEHV_PLAIN>(p, s);
    case SF_TAEHV_RELU: return launch_epi<NT, SF_TAEHV_RELU>(p, s);
    case SF_TAEHV_HEAD_F32: return launch_epi<NT, SF_TAEHV_HEAD_F32>(p, s);
    default: return -1;
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
  SF_CHECK(a->epilogue >= SF_TAEHV_BIAS_RELU && a->epilogue <= SF_TAEHV_HEAD_F32, "sf_taehv_conv: unknown epilogue %d", a->epilogue);
  SF_CHECK(a->Tout > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0, "sf_taehv_conv: empty problem");
  SF_CHECK(a->Cin % 32 == 0, "sf_taehv_conv: Cin=%d must be a multiple of 32 (pad the channels)", a->Cin);
  SF_CHECK(a->kt == 1 || a->kt == 2, "sf_taehv_conv: kt must be 1 or 2, got %d", a->kt);
  SF_CHECK(a->upsample == 0 || a->upsample == 1, "sf_taehv_conv: upsample must be 0 or 1");
  SF_CHECK(!a->upsample || (a->H % 2 == 0 && a->W % 2 == 0), "sf_taehv_conv: an upsampled output %dx%d must be even", a->H, a->W);
  const bool has_bias = a->epilogue == SF_TAEHV_BIAS_RELU || a->epilogue == SF_TAEHV_BIAS_RESID_RELU || a->epilogue == SF_TAEHV_HEAD_F32;
  SF_CHECK(!has_bias || a->bias, "sf_taehv_conv: epilogue %d needs a bias", a->epilogue);
  const int slices = a->kt * 9 * (a->Cin / 32);
  const int nk = (slices + 1) / 2;
  SF_CHECK(a->ldw >= nk * 64 && a->ldw % 8 == 0, "sf_taehv_conv: weight row stride %d < padded K %d", a->ldw, nk * 64);
  SF_CHECK((long)a->Tout * a->H * a->W < (1L << 31), "sf_taehv_conv: too many output positions");
  SF_CHECK(((uintptr_t)a->x % 16 == 0) && ((uintptr_t)a->w % 16 == 0) && ((uintptr_t)a->bias % 8 == 0), "sf_taehv_conv: misaligned tensor");
  const int tgrow = a->tgrow <= 1 ? 1 : a->tgrow;
  SF_CHECK(tgrow <= 2, "sf_taehv_conv: tgrow must be 1 or 2, got %d", a->tgrow);
  if (a->epilogue == SF_TAEHV_HEAD_F32) {
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
  p.tiles_m = (p.M + TBM - 1) / TBM;
  p.tiles_n = (a->Cout + 32 * nt - 1) / (32 * nt);
  hipStream_t s = (hipStream_t)stream;
  int rc = 0;
  switch (nt) {
    case 4: rc = launch_nt<4>(p, a->epilogue, s); break;
    case 2: rc = launch_nt<2>(p, a->epilogue, s); break;
    default: rc = launch_nt<1>(p, a->epilogue, s); break;
  }
  SF_CHECK(rc == 0, "sf_taehv_conv: unknown epilogue %d", a->epilogue);
  SF_HIP_LAUNCH_CHECK("sf_taehv_conv");
  return 0;
}
