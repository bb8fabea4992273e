// The two convolutions of the TAEHV tiny encoder (demo_utils/taehv.py:172-178) that the decoder has no like of, for
// gfx950 (MI355X): the 3 -> 64 stem at full resolution and the stride-2 3x3 with TPool folded in.
//
// sf_taehv_encode_stem replaces encoder.0 + ReLU (taehv.py:173) together with the wrapper's `x * 0.5 + 0.5` (the inverse
// of demo.py:98) and the layout change in front of it.  K = 27 (padded to 32) is ONE 16x16x32 MFMA step per 16 pixels x
// 16 channels; the kernel is a memory-bound writer (128 B out per 6-12 B in), so it reads the caller's planar pixels
// through an LDS halo tile and there is no prepared, padded copy of the input.  A workgroup owns 8 x 32 pixels of one
// frame: the (8+2) x (32+2) x 3 halo goes to LDS as bf16 [row][col][c] -- so that the nine taps (dw, c) of one dh are
// nine consecutive elements, and k = (dh*3+dw)*3 + c -- and each wave takes two rows as four groups of 16 pixels.  The
// rows of the weight fragment are permuted, row 4q + j of channel block cb holding channel 16q + 4cb + j: the lane
// that holds rows 4q .. 4q+3 of the four results then owns 16 CONSECUTIVE channels of its pixel (32 B), and the four
// lanes of a pixel write its whole 128-byte row.
//
// sf_taehv_down_conv is TPool(64, s) + conv(64, 64, stride=2) as one convolution with s temporal taps at temporal stride s
// (taehv_weights.fold_tpool): an instantiation of conv_igemm_core.h with stride_hw() = 2 and stride_t() = kt as
// compile-time constants; gather, main loop and epilogue are the core's.
#include <cstdlib>
#include "conv_igemm_core.h"
#include "../../include/sf_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------ the stem
constexpr int ST_TH = 8, ST_TW = 32;                 // pixels of a workgroup's tile
constexpr int ST_HH = ST_TH + 2, ST_HW = ST_TW + 2;  // with the halo
constexpr int ST_ELEMS = ST_HH * ST_HW * 3;

template <typename PixT>
__global__ __launch_bounds__(256) void taehv_stem_kernel(const PixT* __restrict__ pix, long c_stride, int H, int W, int lead, int tiles_x, int tiles_y,
                                                         const bf16_t* __restrict__ w, const bf16_t* __restrict__ bias, bf16_t* __restrict__ out) {
  __shared__ bf16_t tile[ST_ELEMS + 8];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per_frame = tiles_x * tiles_y;
  const int t = blockIdx.x / per_frame, rem = blockIdx.x - t * per_frame;
  const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
  const int y0 = ty * ST_TH, x0 = tx * ST_TW;
  const int src = max(t - lead, 0);                  // the front padding: the first frame `lead` more times

  // the lane's weight fragments and bias: independent of the tile, requested before the halo
  const int i16 = lane & 15, kq = lane >> 4;
  bf16x8 wf[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) wf[cb] = *reinterpret_cast<const bf16x8*>(w + (16 * (i16 >> 2) + 4 * cb + (i16 & 3)) * 32 + 8 * kq);
  const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(bias + 16 * kq), b1 = *reinterpret_cast<const bf16x8*>(bias + 16 * kq + 8);

  // halo tile: u = 0.5 x + 0.5 rounded to bf16 inside the image, 0 outside (the convolution's zero padding)
  for (int i = tid; i < ST_ELEMS; i += 256) {
    const int c = i / (ST_HH * ST_HW), r = i - c * (ST_HH * ST_HW);
    const int yy = r / ST_HW, xx = r - yy * ST_HW;
    const int gy = y0 + yy - 1, gx = x0 + xx - 1;
    float v = 0.f;
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) v = 0.5f * (float)pix[c * c_stride + ((long)src * H + gy) * W + gx] + 0.5f;
    tile[(yy * ST_HW + xx) * 3 + c] = (bf16_t)v;
  }
  __syncthreads();

  // element offsets of the lane's eight k = 8 kq + i inside a pixel's window (k >= 27: the padding of K, read as zero)
  int koff[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = 8 * kq + i, dh = k / 9;
    koff[i] = k < 27 ? dh * (ST_HW * 3) + (k - 9 * dh) : 0;
  }
  const int kvalid = 27 - 8 * kq;   // the lane's first `kvalid` elements are real taps
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int row = wave * 2 + (g >> 1), col = (g & 1) * 16 + i16;
    const int base = (row * ST_HW + col) * 3;
    bf16x8 xf;
#pragma unroll
    for (int i = 0; i < 8; ++i) xf[i] = i < kvalid ? tile[base + koff[i]] : (bf16_t)0.f;
    f32x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cb], xf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    // acc[cb][j] = channel 16 kq + 4 cb + j of pixel (row, col)
    bf16x8 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o0[j] = (bf16_t)fmaxf(acc[0][j] + (float)b0[j], 0.f);
      o0[4 + j] = (bf16_t)fmaxf(acc[1][j] + (float)b0[4 + j], 0.f);
      o1[j] = (bf16_t)fmaxf(acc[2][j] + (float)b1[j], 0.f);
      o1[4 + j] = (bf16_t)fmaxf(acc[3][j] + (float)b1[4 + j], 0.f);
    }
    const int gy = y0 + row, gx = x0 + col;
    if (gy < H && gx < W) {
      bf16_t* dst = out + (((long)t * H + gy) * W + gx) * 64 + 16 * kq;
      *reinterpret_cast<bf16x8*>(dst) = o0;
      *reinterpret_cast<bf16x8*>(dst + 8) = o1;
    }
  }
}

// ------------------------------------------------------------------------------- the strided convolution
template <int KT>
struct TDownP {
  const bf16_t* x;
  const bf16_t* w;
  const bf16_t* bias;    // (the core's epilogue names them; PLAIN reads neither)
  bf16_t* out;
  const bf16_t* resid;
  int M, HW, H, W;
  int Hin, Win;
  int Cin, Cout, cpt, ntaps;
  int nk, ldw, ldo, ldr;
  int tiles_m, tiles_n;
  unsigned x_bytes;
  static constexpr int up = 0;
  // what conv_igemm_core.h asks of its caller: 3x3 at spatial stride 2, padded by 1, kt taps at temporal stride kt
  __device__ __forceinline__ static constexpr int stride_hw() { return 2; }
  __device__ __forceinline__ static constexpr int stride_t() { return KT; }
  __device__ __forceinline__ static constexpr int pad_h() { return 1; }
  __device__ __forceinline__ static constexpr int pad_w() { return 1; }
  __device__ __forceinline__ int tap_h() const { return Hin; }
  __device__ __forceinline__ int tap_w() const { return Win; }
  __device__ __forceinline__ static constexpr int frame_off() { return 0; }
  __device__ __forceinline__ static constexpr bool spatial3x3() { return true; }
  __device__ __forceinline__ static constexpr long resid_row0() { return 0; }
  __device__ __forceinline__ void store(int m, int n, const bf16x8& v) const { *reinterpret_cast<bf16x8*>(out + (long)m * ldo + n) = v; }
};

template <int KT>
__global__ __launch_bounds__(igemm::THREADS, 2) void taehv_down_conv_kernel(TDownP<KT> p) {
  constexpr int NT = 2;
  constexpr int BN = 32 * NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wg = sf_xcd_remap(bid, nwg);
  const int tm = wg / p.tiles_n, tn = wg - tm * p.tiles_n;
  const int m0 = tm * igemm::BM, n0 = tn * BN;

#include "conv_igemm_mainloop.inc"

  constexpr bool EPI_BIAS = false, EPI_RESID = false, EPI_RELU = false;
#include "conv_igemm_epilogue.inc"
}

template <int KT>
int launch_down(const sf_taehv_down_conv_args* a, int nk, unsigned x_bytes, hipStream_t s) {
  constexpr int NT = 2;
  constexpr int LDS = igemm::lds_bytes(NT);
  static_assert(LDS <= 64 * 1024, "the tiles of this kernel fit the default dynamic-LDS limit");
  static_assert(igemm::BM * igemm::out_row_bytes(NT) <= LDS, "the epilogue's output tile fits the stages");
  TDownP<KT> p;
  p.x = (const bf16_t*)a->x; p.w = (const bf16_t*)a->w; p.bias = nullptr; p.out = (bf16_t*)a->out; p.resid = nullptr;
  p.HW = a->H * a->W; p.M = a->Tout * p.HW; p.H = a->H; p.W = a->W;
  p.Hin = 2 * a->H; p.Win = 2 * a->W;
  p.Cin = a->Cin; p.Cout = a->Cout; p.cpt = a->Cin / 32; p.ntaps = KT * 9;
  p.nk = nk; p.ldw = a->ldw; p.ldo = a->ldo; p.ldr = 0;
  p.tiles_m = (p.M + igemm::BM - 1) / igemm::BM;
  p.tiles_n = a->Cout / (32 * NT);
  p.x_bytes = x_bytes;
  return sf_launch<&taehv_down_conv_kernel<KT>>("sf_taehv_down_conv", dim3(p.tiles_m * p.tiles_n), dim3(igemm::THREADS), LDS, s, p);
}

}  // namespace

extern "C" int sf_taehv_encode_stem(const void* pixels, int dtype, int64_t c_stride, int H, int W, int n_frames, int lead, const void* w, const void* bias,
                                    void* out, void* stream) {
  SF_CHECK(pixels && w && bias && out, "sf_taehv_encode_stem: null tensor");
  SF_CHECK(dtype == SF_TAEHV_PIXEL_BF16 || dtype == SF_TAEHV_PIXEL_F32, "sf_taehv_encode_stem: unknown pixel dtype %d", dtype);
  SF_CHECK(H > 0 && W > 0 && H <= 32768 && W <= 32768 && n_frames > 0 && n_frames <= 4096, "sf_taehv_encode_stem: %d frames of %dx%d", n_frames, H, W);
  SF_CHECK(lead >= 0 && lead <= 3 && lead < n_frames, "sf_taehv_encode_stem: lead=%d (0..3, below n_frames=%d)", lead, n_frames);
  SF_CHECK(c_stride >= (int64_t)(n_frames - lead) * H * W, "sf_taehv_encode_stem: channel stride %lld < %d frames of %dx%d", (long long)c_stride,
           n_frames - lead, H, W);
  SF_CHECK((uintptr_t)w % 16 == 0 && (uintptr_t)bias % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)pixels % (dtype == SF_TAEHV_PIXEL_F32 ? 4 : 2) == 0,
           "sf_taehv_encode_stem: misaligned tensor");
  const int tiles_x = (W + ST_TW - 1) / ST_TW, tiles_y = (H + ST_TH - 1) / ST_TH;
  const long blocks = (long)tiles_x * tiles_y * n_frames;
  SF_CHECK(blocks < (1L << 31), "sf_taehv_encode_stem: too many tiles");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  if (dtype == SF_TAEHV_PIXEL_F32)
    return sf_launch<&taehv_stem_kernel<float>>("sf_taehv_encode_stem", grid, block, 0, s, (const float*)pixels, (long)c_stride, H, W, lead, tiles_x, tiles_y,
                                                (const bf16_t*)w, (const bf16_t*)bias, (bf16_t*)out);
  return sf_launch<&taehv_stem_kernel<bf16_t>>("sf_taehv_encode_stem", grid, block, 0, s, (const bf16_t*)pixels, (long)c_stride, H, W, lead, tiles_x, tiles_y,
                                               (const bf16_t*)w, (const bf16_t*)bias, (bf16_t*)out);
}

extern "C" int sf_taehv_down_conv(const sf_taehv_down_conv_args* a, void* stream) {
  SF_CHECK(a != nullptr, "sf_taehv_down_conv: null args");
  SF_CHECK(a->x && a->w && a->out, "sf_taehv_down_conv: null tensor");
  SF_CHECK(a->Tout > 0 && a->H > 0 && a->W > 0 && a->H <= 16384 && a->W <= 16384 && a->Cin > 0 && a->Cout > 0, "sf_taehv_down_conv: empty problem");
  SF_CHECK(a->Cin % 32 == 0, "sf_taehv_down_conv: Cin=%d must be a multiple of 32 (pad the channels)", a->Cin);
  SF_CHECK(a->Cout % 64 == 0, "sf_taehv_down_conv: Cout=%d must be a multiple of 64", a->Cout);
  SF_CHECK(a->kt == 1 || a->kt == 2, "sf_taehv_down_conv: kt must be 1 or 2, got %d", a->kt);
  const int slices = a->kt * 9 * (a->Cin / 32);
  const int nk = (slices + 1) / 2;
  SF_CHECK(a->ldw >= nk * 64 && a->ldw % 8 == 0, "sf_taehv_down_conv: weight row stride %d < padded K %d", a->ldw, nk * 64);
  SF_CHECK(a->ldo >= a->Cout && a->ldo % 8 == 0, "sf_taehv_down_conv: ldo %d too small for %d channels / ldo %% 8 != 0", a->ldo, a->Cout);
  SF_CHECK((long)a->Tout * a->H * a->W < (1L << 31), "sf_taehv_down_conv: too many output positions");
  SF_CHECK(((uintptr_t)a->x % 16 == 0) && ((uintptr_t)a->w % 16 == 0) && ((uintptr_t)a->out % 16 == 0), "sf_taehv_down_conv: misaligned tensor");
  // frames [0, kt * Tout) of the input volume can be gathered from
  const long xb = (long)a->kt * a->Tout * (2L * a->H) * (2L * a->W) * a->Cin * 2;
  SF_CHECK(xb < 0xFFFFFF00L, "sf_taehv_down_conv: input volume of %ld bytes exceeds the 4 GiB the gather's 32-bit offsets cover", xb);
  hipStream_t s = (hipStream_t)stream;
  return a->kt == 2 ? launch_down<2>(a, nk, (unsigned)xb, s) : launch_down<1>(a, nk, (unsigned)xb, s);
}
