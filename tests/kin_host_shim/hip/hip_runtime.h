// Host stand-in for <hip/hip_runtime.h>, for tests/kin_host_driver.cpp only: the kernel source of csrc/snpm_k_kin.hpp is compiled
// for the CPU with this file in the place of the HIP header.  A block is run by 256 real threads (one per GPU thread), blocks one
// after the other; `__shared__` arrays are function statics, `__syncthreads` is a barrier of the 256, `__ballot` exchanges the
// predicates of the 64 threads of a wave.  The driver defines what is declared here.
#pragma once
#include <stdint.h>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static
#define __launch_bounds__(...)

struct kin_dim3 {
    unsigned x, y, z;
};
extern thread_local kin_dim3 threadIdx, blockIdx;

struct alignas(16) uint4 {
    uint32_t x, y, z, w;
};

void __syncthreads();
unsigned long long __ballot(int predicate);
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int atomicAdd(int32_t *p, int32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
