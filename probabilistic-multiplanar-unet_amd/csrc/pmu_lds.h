// LDS / MFMA primitives shared by the kernels that issue their LDS reads and LDS-DMA by hand (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// f32 MFMA D[16x16] += A[16x4] * B[4x16]: lane l supplies A[l&15][l>>4] and B[l>>4][l&15]
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// LDS reads as explicit instructions (the compiler neither merges them into ds_read2 forms nor inserts
// waits for them: the caller waits with wait_lgkm); addr = LDS byte address (lds_addr), OFF = immediate
// byte offset
__device__ __forceinline__ unsigned lds_addr(const float* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) float*)(p);
}
template <int OFF>
__device__ __forceinline__ float lds_b32(unsigned addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ float2 lds_b64(unsigned addr) {
  float2 v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ float4 lds_b128(unsigned addr) {
  float4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
// s_waitcnt lgkmcnt(N) (vmcnt / expcnt left at their maxima; gfx9 encoding)
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  static_assert(N >= 0 && N <= 15, "lgkmcnt");
  __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8));
}

// LDS-DMA of one 16-B unit per lane: global S -> LDS D (no registers, no VALU; waited for with vmcnt)
#define PMU_GLDS(S, D)                                                                                      \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(S),                     \
                                   (__attribute__((address_space(3))) void*)(D), 16, 0, 0);
