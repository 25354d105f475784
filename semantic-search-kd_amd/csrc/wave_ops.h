// Wave-level helpers that more than one translation unit uses (internal: not installed): no LDS, no workgroup barrier.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// sum / maximum over the lanes of one wave
template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// what lanes of a wave wrote to LDS is read by the other lanes of that wave (no workgroup barrier needed)
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// a value every lane holds alike, moved into scalar registers
__device__ inline int64_t wave_uniform(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// LDS-DMA: 16 B per lane, global -> LDS, no registers (LDS address = wave-uniform base + 16 lane)
__device__ inline void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

}  // namespace
