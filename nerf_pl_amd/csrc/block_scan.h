// What the one-workgroup passes of the mesh kernels (mesh.hip), the volume export (volume.hip) and the GIF and PNG encoders (gif.hip,
// png.hip) share: the workgroup-wide exclusive scan, the offsets scan over more values than the workgroup has threads, and the
// carving of a workspace into 256-byte aligned arrays.
#pragma once
#include <hip/hip_runtime.h>

namespace nerfhip {

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The next array of a workspace: `count` elements of T at the cursor, which advances by their bytes rounded up to 256.  A layout
// carved from a null base leaves its size in the cursor: the size query and the launch read the same lines.
template <typename T>
__host__ __device__ inline T* carve(char*& cursor, size_t count) {
    T* const at = (T*)cursor;
    cursor += align256(count * sizeof(T));
    return at;
}

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

// Exclusive offsets of the n values value(0) .. value(n - 1) by one workgroup of NT threads: off[i] = value(0) + ... + value(i - 1),
// in passes of NT values with the sum so far carried from pass to pass.  Every thread gets the sum of all n.  value(i) is called
// once for every i < n, by thread i % NT; all threads of the workgroup must call this together.  with_pass(i) runs in every thread
// behind each pass, also for i >= n in the last one, and may hold workgroup-wide steps of its own (png_scan: the Adler sums).
struct NoPassStep { __device__ __forceinline__ void operator()(int64_t) const {} };

template <int NT, typename F, typename G = NoPassStep>
__device__ __forceinline__ int64_t block_offsets_scan(int64_t n, int64_t* __restrict__ off, F value, G with_pass = G()) {
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += NT) {
        const int64_t i = base + threadIdx.x;
        int64_t tot;
        const int64_t ex = block_excl_scan<NT>(i < n ? (int64_t)value(i) : (int64_t)0, tot);
        if (i < n) off[i] = carry + ex;
        carry += tot;
        with_pass(i);
    }
    return carry;
}

}  // namespace nerfhip
