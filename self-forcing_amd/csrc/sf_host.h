// Internal scaffold shared by the host sequencers (dit_forward, t5_encoder, vae_decode / vae_encode through vae_common.h,
// taehv_decode, pose_embed): workspace carving, error propagation, and the one way to issue a GEMM.  The frame and
// keypoint entry points (jpeg, jpeg_decode, resize, pose_render / retarget / smooth / track / estimate, sf_pose_prepare)
// include sf_frame_host.h, which brings this file and adds their own shared pieces (strides, ranges, the pixel-type
// dispatch, keypoint constants).  Host-side only; not part of include/sf_hip.h.
#pragma once
#include <cstring>
#include "sf_common.h"
#include "../../include/sf_hip.h"

// a failed hipMemsetAsync / hipMemcpyAsync as the library's error return: "<who>: <what> failed: <hip's words>"
inline int sf_hip_ok(hipError_t e, const char* who, const char* what) {
  SF_CHECK(e == hipSuccess, "%s: %s failed: %s", who, what, hipGetErrorString(e));
  return 0;
}

// 256-byte-aligned carving of a caller's block; over a null base it only measures (the *_bytes functions)
struct Carve {
  char* base;
  size_t off;
  explicit Carve(void* p) : base((char*)p), off(0) {}
  char* take(size_t bytes) {
    char* r = base ? base + off : nullptr;
    off += (bytes + 255) & ~(size_t)255;
    return r;
  }
};

// One sf_gemm_bf16 / sf_gemm_fp8 call: out [M, N] = a [M, K] . w [N, K]^T.  Only the operand geometry is positional;
// everything optional is named at the call site, so two trailing ints cannot trade places unnoticed:
//   Gemm(a, lda, w, ldw, out, ldo, M, N, K).bias(b).epi(SF_EPI_BIAS_RESID).resid(x, ldr).bf16(stream)
struct Gemm {
  sf_gemm_args g;
  const void* wq = nullptr;        // the fp8 twin of w and its column scales (fp8w)
  const float* w_scale = nullptr;
  int rows_per_segment = 0;
  Gemm(const void* a, int lda, const void* w, int ldw, void* out, int ldo, int M, int N, int K) {
    memset(&g, 0, sizeof(g));
    g.a = a; g.lda = lda; g.w = w; g.ldw = ldw; g.out = out; g.ldo = ldo; g.M = M; g.N = N; g.K = K;
    g.epilogue = SF_EPI_BIAS;
    g.rows_per_group = 1;
  }
  Gemm& bias(const void* b) { g.bias = b; return *this; }
  Gemm& epi(int e) { g.epilogue = e; return *this; }
  Gemm& resid(const void* r, int ldr) { g.resid = r; g.ldr = ldr; return *this; }
  // SF_EPI_BIAS_GATE_RESID: y * (gate_mod[n] + gate_e0[m / rows_per_group][n]), gate_e0's rows `group_stride` apart
  Gemm& gate(const void* gate_mod, const void* gate_e0, long group_stride, int rows_per_group) {
    g.gate_mod = gate_mod; g.gate_e0 = gate_e0; g.gate_group_stride = group_stride; g.rows_per_group = rows_per_group;
    return *this;
  }
  Gemm& batch(int n, long a_bstride, long w_bstride, long o_bstride) {
    g.batch = n; g.a_bstride = a_bstride; g.w_bstride = w_bstride; g.o_bstride = o_bstride;
    return *this;
  }
  // the e4m3 weight [N, K] that fp8() reads in place of w, its fp32 column scales, and the rows that share one
  // activation scale
  Gemm& fp8w(const void* w_e4m3, const float* scale, int rows_per_seg) {
    wq = w_e4m3; w_scale = scale; rows_per_segment = rows_per_seg;
    return *this;
  }
  int bf16(void* stream) const { return sf_gemm_bf16(&g, stream); }
  // the same product on e4m3 operands: aq = sf_quantize_fp8 of a (dense rows of K), a_scale its scales
  int fp8(const void* aq, const float* a_scale, void* stream) const {
    sf_gemm_args q = g;
    q.a = aq; q.lda = g.K; q.w = wq;
    return sf_gemm_fp8(&q, a_scale, rows_per_segment, w_scale, stream);
  }
};

// One sf_attention call, in the same style: each operand with its token and batch stride, then the problem size;
// everything optional is named:
//   Attention(q, q_stride, q_bstride, k, v, kv_stride, kv_bstride, out, o_stride, o_bstride, B, H, Lq, Lk).fold(keys, log2w).run(stream)
struct Attention {
  sf_attention_args a;
  Attention(const void* q, long q_stride, long q_bstride, const void* k, const void* v, long kv_stride, long kv_bstride, void* out,
            long o_stride, long o_bstride, int B, int H, int Lq, int Lk) {
    memset(&a, 0, sizeof(a));
    a.q = q; a.q_stride = q_stride; a.q_bstride = q_bstride;
    a.k = k; a.v = v; a.kv_stride = kv_stride; a.kv_bstride = kv_bstride;
    a.out = out; a.o_stride = o_stride; a.o_bstride = o_bstride;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
    a.structure = SF_ATTN_AUTO;
  }
  Attention& structure(int s) { a.structure = s; return *this; }
  Attention& accum() { a.accumulate = 1; return *this; }                  // out += the attention
  Attention& fold(const int32_t* keys, const float* log2w) { a.keys = keys; a.log2w = log2w; return *this; }
  int run(void* stream) const { return sf_attention(&a, stream); }
};
