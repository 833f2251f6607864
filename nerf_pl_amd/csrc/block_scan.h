// The workgroup-wide exclusive scan shared by the mesh kernels (mesh.hip) and the GIF encoder (gif.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace nerfhip {

// Exclusive scan of one value per thread over a block of NT threads (NT/64 waves): returns the thread's exclusive prefix,
// `total` gets the block's sum.  Callable once per __syncthreads-separated phase.
template <int NT, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T& total) {
    __shared__ T wsum[NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        T t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const T s = wsum[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();
    total = all;
    return before + incl - v;
}

}  // namespace nerfhip
