// What every split-precision engine shares (conv3_common.h: the 3x3 kernels; gemm_plane.h: the GEMM engines; stem.hip): the fragment type,
// the scale of the lo' plane, the LDS slot swizzle and the LDS-DMA helpers -- one copy each.
#pragma once
#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float LO_UNSCALE = 1.0f / 1024.0f;           // x = hi + lo' / 1024

// 16-byte slot swizzle of the 64-byte LDS rows
__device__ __forceinline__ int swz64(int row) { return ((row >> 2) & 1) << 1; }
// one LDS-DMA piece: 16 bytes per lane from `src` (per lane) to wave-uniform base + lane * 16 B
__device__ __forceinline__ void dma16(const unsigned char* src, unsigned char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
