// Host stand-in for <hip/hip_runtime.h>: the kernel source of a csrc/snpm_k_*.hpp family header is compiled for the CPU with this file
// in the place of the HIP header (tests/kin_host_driver.cpp, tests/site_host_driver.cpp).  A block is run by one real thread per GPU
// thread, blocks one after the other; `__shared__` arrays are function statics, `__syncthreads` is a barrier of the block, `__ballot`
// and `__shfl_xor` exchange a value among the 64 threads of a wave.  tests/host_kernel/harness.hpp defines what is declared here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static
#define __launch_bounds__(...)

struct host_dim3 {
    unsigned x, y, z;
};
extern thread_local host_dim3 threadIdx, blockIdx, gridDim;

struct alignas(16) uint4 {
    uint32_t x, y, z, w;
};
struct alignas(16) int4 {
    int x, y, z, w;
};

void __syncthreads();
unsigned long long __ballot(int predicate);
uint32_t __shfl_xor(uint32_t value, int lane_mask);
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int atomicAdd(int32_t *p, int32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
