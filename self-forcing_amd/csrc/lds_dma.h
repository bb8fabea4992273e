// Global -> LDS copies without a register round trip (LDS-DMA): the flat form (gemm_bf16.hip, conv_halo.hip's weights, the
// W tiles of conv_igemm_core.h), and the range-checked buffer form whose out-of-range lanes write zeros to LDS (the
// gathered A tiles of conv_igemm_core.h, i.e. conv_igemm.hip and taehv_conv.hip, and conv_halo.hip's planes).
#pragma once
#include "sf_common.h"

#ifdef __HIPCC__
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// 16 bytes per lane: lane l's piece lands at lds_wave_base + 16 l
__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_wave_base, 16, 0, 0);
}

// raw buffer descriptor over [base, base + bytes): byte offsets >= bytes read as zero
__device__ __forceinline__ u32x4 lds_dma_srd(const void* base, unsigned bytes) {
  const unsigned long long a64 = (unsigned long long)base;
  u32x4 srd;
  srd[0] = __builtin_amdgcn_readfirstlane((unsigned)a64);
  srd[1] = __builtin_amdgcn_readfirstlane((unsigned)(a64 >> 32) & 0xFFFFu);
  srd[2] = __builtin_amdgcn_readfirstlane(bytes);
  srd[3] = 0x00020000u;
  return srd;
}

// 16 bytes per lane from byte offset `voff` of the descriptor to lds_addr + 16 lane (lds_addr wave-uniform)
__device__ __forceinline__ void lds_dma16_checked(u32x4 srd, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 4\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(lds_addr), "v"(voff), "s"(srd) : "memory");
}
#endif
