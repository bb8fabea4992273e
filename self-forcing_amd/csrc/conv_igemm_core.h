// The implicit-GEMM convolution core shared by conv_igemm.hip (Wan VAE) and taehv_conv.hip (TAEHV): a GEMM with
// M = Tout*H*W output positions, N = Cout, K = taps*Cin whose A operand is gathered by the range-checked LDS-DMA;
// 128 x (32 NT) output tile per 256-thread workgroup, 4 waves as 2x2, two LDS stages.  Device code only.
//
//   conv_igemm_core.h         the tile constants (this file)
//   conv_igemm_mainloop.inc   the per-lane piece set-up, the slice cursor with gather_offsets, the fragment addresses,
//                             the prologue and the 4 + NT-slice k-loop: fills f32x4 acc[4][NT] for the tile at (m0, n0)
//   conv_igemm_epilogue.inc   the through-LDS bf16 epilogue: bias / residual / ReLU by compile-time flags, staging into
//                             16-byte-padded rows, write-back in 16-byte pieces through the kernel's store
//
// The two .inc files are the TEXT of a kernel body, included where a call would stand.  As __forceinline__ templates
// they compile to different code: the compiler simplifies a callee on its own before it inlines it, with the tile
// origin, the wave number and the parameter struct opaque, and does not find its way back (the mask loop is no
// longer vectorised, registers move in every instantiation; even the swizzle as a one-line helper moves 2.7 k lines
// of conv_igemm's assembly).  As text conv_igemm.hip compiles to the instructions it had with its own copy.
//
// What differs between the callers the kernel's parameter struct answers through inline members -- run-time fields for
// the VAE, compile-time constants for TAEHV, whose tap arithmetic then folds to the shorter form:
//   stride_hw(), stride_t()   spatial / temporal input stride
//   pad_h(), pad_w()          zero padding in front
//   tap_h(), tap_w()          bounds of the tap coordinates
//   frame_off()               input frame under output frame 0's first temporal tap
//   spatial3x3()              3x3 spatial taps (else 1x1)
//   resid_row0(), store()     the epilogue's residual origin and output layout (conv_igemm_epilogue.inc)
#pragma once
#include "lds_dma.h"

namespace igemm {

constexpr int BM = 128, BK = 64;
constexpr int THREADS = 256;
constexpr int A_TILE_BYTES = BM * BK * 2;   // 16 KiB
constexpr int stage_bytes(int NT) { return A_TILE_BYTES + 32 * NT * BK * 2; }   // A tile + W tile
constexpr int lds_bytes(int NT) { return 2 * stage_bytes(NT); }                 // two stages
constexpr int out_row_bytes(int NT) { return 64 * NT + 16; }                    // a padded row of the epilogue's staging image

}  // namespace igemm
