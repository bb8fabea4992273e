// The through-LDS bf16 epilogue of the implicit-GEMM convolutions, included into the kernel body by conv_igemm.hip and
// taehv_conv.hip behind conv_igemm_mainloop.inc (see conv_igemm_core.h for why this is text and not a function).
//
// The 128 x BN tile is assembled as bf16 rows (padded by 16 B against bank conflicts) and written back in 16-byte pieces
// along the rows -- with all channels in one tile that is one contiguous region of the output volume.  The direct form
// stores 8-byte pieces of 16 different positions per instruction (32-byte partial lines): a quarter of HBM's write
// efficiency on the 300 MB volumes.
//
// Expects in scope: what conv_igemm_mainloop.inc expects and leaves behind, tid, and the compile-time flags EPI_BIAS,
// EPI_RESID, EPI_RELU: y = acc (+ bias) (+ residual), ReLU or not, rounded once.  The parameter struct adds the fields
// bias, resid, ldr and two inline members: resid_row0(), the residual row of output position 0, and
// store(m, n, v), which writes the eight channels n .. n + 7 of output position m (m < M, n < Cout).
  constexpr int RBP = igemm::out_row_bytes(NT);   // padded row bytes
  char* obuf = smem;                   // (the k-loop's last __syncthreads has released the stages)
  // bias and residual are requested for the whole wave tile first and consumed afterwards (one memory round trip
  // instead of 4 NT dependent ones, see gemm_epilogue_lds)
  int ncol[NT];
  bf16x4 bias_v[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    ncol[nt] = min(n0 + wc * (16 * NT) + nt * 16 + (lane >> 4) * 4, p.Cout - 4);
    if (EPI_BIAS) bias_v[nt] = *reinterpret_cast<const bf16x4*>(p.bias + ncol[nt]);
  }
  bf16x4 rv[4][NT];
  if (EPI_RESID) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = min(m0 + wr * 64 + mt * 16 + (lane & 15), p.M - 1);
      const long grow = p.resid_row0() + m;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) rv[mt][nt] = *reinterpret_cast<const bf16x4*>(p.resid + grow * p.ldr + ncol[nt]);
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
      if (EPI_BIAS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] += (float)bias_v[nt][j];
      }
      if (EPI_RESID) {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] += (float)rv[mt][nt][j];
      }
      if (EPI_RELU) {
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
  for (int i = 0; i < (igemm::BM * CPR) / igemm::THREADS; ++i) {
    const int id = i * igemm::THREADS + tid;
    const int row = id / CPR, ch = id - row * CPR;
    const int m = m0 + row, n = n0 + ch * 8;
    if (m < p.M && n < p.Cout) p.store(m, n, *reinterpret_cast<const bf16x8*>(obuf + row * RBP + ch * 16));
  }
