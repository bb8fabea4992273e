// The gather and main loop of the implicit-GEMM convolutions, included into the kernel body by conv_igemm.hip and
// taehv_conv.hip (see conv_igemm_core.h for why this is text and not a function).
//
// Expects in scope: NT; the parameter struct p with the fields x, w, M, HW, W, Hin, Win, up, Cin, Cout, cpt, ntaps, nk,
// ldw, x_bytes and the geometry accessors of conv_igemm_core.h; smem (the dynamic LDS); lane, wave; the tile origin m0, n0.
// Leaves behind: wr, wc (the wave's row / column in the 2 x 2 wave grid) and f32x4 acc[4][NT], the lane holding
// out[m][n .. n+3] for (mt, nt) with m = m0 + wr * 64 + 16 mt + (lane & 15), n = n0 + wc * 16 NT + 16 nt + 4 (lane >> 4);
// the last __syncthreads has released the stages.

  constexpr int STAGE = igemm::stage_bytes(NT);
  // ---- the four A pieces of this lane: row r of the tile, 16-byte chunk c of the 128-byte LDS row (chunks 0-3 hold
  // the first 32-channel slice of the k-step, 4-7 the second).  Everything that does not depend on the tap is
  // computed ONCE: the byte offset of the piece at tap (0, 0, 0) and a 9-bit mask of the spatial taps that fall
  // inside the image.  Per k-step a piece then costs a handful of VALU instructions: offset = base + D(slice) with D
  // wave-uniform, validity = one bit of the mask, and an invalid piece (zero padding, rows past M, the padding slice
  // of an odd slice count) gets an out-of-range offset: the range-checked buffer load writes zeros to LDS.
  unsigned abase[4], vmask[4], parh[4], parw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);   // the chunk swizzle (written out: behind a helper the set-up compiles differently)
    const int m = m0 + r;
    const bool valid = m < p.M;
    const int mm = min(m, p.M - 1);
    const int t = mm / p.HW, hw = mm - t * p.HW;
    const int h = hw / p.W;
    const int hh0 = h * p.stride_hw() - p.pad_h(), ww0 = (hw - h * p.W) * p.stride_hw() - p.pad_w();
    abase[i] = (unsigned)(((((long)(t * p.stride_t() + p.frame_off()) * p.Hin + (hh0 >> p.up)) * p.Win + (ww0 >> p.up)) * p.Cin + (c & 3) * 8) * 2);
    unsigned vm = 0;
    const int kk = p.spatial3x3() ? 3 : 1;
    for (int dh = 0; dh < kk; ++dh)
      for (int dw = 0; dw < kk; ++dw)
        if (valid && (unsigned)(hh0 + dh) < (unsigned)p.tap_h() && (unsigned)(ww0 + dw) < (unsigned)p.tap_w()) vm |= 1u << (dh * 3 + dw);
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
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int n = min(n0 + r, p.Cout - 1);
    w_src[j] = p.w + (long)n * p.ldw + c * 8;
  }
  // range-checked view of the input volume (offsets past x_bytes read as zero)
  const u32x4 x_srd = lds_dma_srd(p.x, p.x_bytes);
  const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) char*)smem;

  // slice cursor of the NEXT stage to issue: slice 2 kt = (tap, cc), cc counting 32-channel groups
  int tap = 0, cc = 0;
  const unsigned rowB = (unsigned)(p.Win * p.Cin * 2), colB = (unsigned)(p.Cin * 2), frameB = (unsigned)(p.Hin * p.Win * p.Cin * 2);
  // byte offsets of this lane's four A pieces of the stage the cursor points at; advances the cursor
  auto gather_offsets = [&](unsigned (&voff)[4]) __attribute__((always_inline)) {
    int tap1 = tap, cc1 = cc + 1;
    if (cc1 >= p.cpt) { cc1 -= p.cpt; ++tap1; }
    int dt0, dh0, dw0, dt1, dh1, dw1;   // tap -> (dt, dh, dw), tap < 32: 3x3 or 1x1 spatial taps
    if (p.spatial3x3()) {
      dt0 = (tap * 57) >> 9; const int r0 = tap - 9 * dt0; dh0 = (r0 * 11) >> 5; dw0 = r0 - 3 * dh0;
      dt1 = (tap1 * 57) >> 9; const int r1 = tap1 - 9 * dt1; dh1 = (r1 * 11) >> 5; dw1 = r1 - 3 * dh1;
    } else {
      dt0 = tap; dh0 = dw0 = 0; dt1 = tap1; dh1 = dw1 = 0;
    }
    const unsigned sh0 = tap < p.ntaps ? (unsigned)(dh0 * 3 + dw0) : 31u, sh1 = tap1 < p.ntaps ? (unsigned)(dh1 * 3 + dw1) : 31u;
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
  const int w_row_off = igemm::A_TILE_BYTES + (wc * (16 * NT) + i16) * 128;       // + nt*2048
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
    char* wbase = smem + igemm::A_TILE_BYTES + wave * (NT * 1024);
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
    // The k-step as 4 + NT pinned slices of {MFMAs of the first 32-deep sub-step, one fragment read of the second,
    // ONE LDS-DMA request of the next stage} (see gemm_bf16.hip), then the second sub-step's MFMAs, under which the
    // gather offsets of the stage after next are computed.  The last k-step re-requests its own W pieces and
    // all-invalid A pieces into the idle buffer so that the body stays branch-free.
    const unsigned abase_lds = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)((cur ^ 1) * STAGE + wave * 4096));
    char* wbase = smem + (cur ^ 1) * STAGE + igemm::A_TILE_BYTES + wave * (NT * 1024);
    const int kn = min(kt + 1, p.nk - 1) * igemm::BK;
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
