// Host stand-in for <hip/hip_runtime.h>, for tests/site_host_driver.cpp only: the kernel source of csrc/snpm_k_site.hpp is compiled
// for the CPU with this file in the place of the HIP header.  A block is run by 512 real threads (one per GPU thread), blocks one
// after the other; `__shared__` arrays are function statics, `__syncthreads` is a barrier of the 512, `__shfl_xor` exchanges a value
// among the 64 threads of a wave.  The driver defines what is declared here.
#pragma once
#include <stdint.h>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static
#define __launch_bounds__(...)

struct site_dim3 {
    unsigned x, y, z;
};
extern thread_local site_dim3 threadIdx, blockIdx, gridDim;

struct alignas(16) uint4 {
    uint32_t x, y, z, w;
};
struct alignas(16) int4 {
    int x, y, z, w;
};

void __syncthreads();
uint32_t __shfl_xor(uint32_t value, int lane_mask);
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
