// The launch side of a twin (twin.h): a unit writes one item operation — a struct that holds the unit's arguments and output
// pointers and whose operator()(int64_t i) does item i's load, core routine and stores, optional outputs included — and both its
// one-thread-per-item kernel (item_index, bound check, op(i)) and its _host entry point (host_items) call that.
#pragma once
#include "common.h"

namespace nerfhip {

constexpr int kItemBlock = 256;                   // threads per block of every one-thread-per-item launch
constexpr int64_t kMaxRays = (int64_t)1 << 30;    // rows per call of a ray unit

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kItemBlock - 1) / kItemBlock); }
inline bool misaligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) != 0; }

__device__ __forceinline__ int64_t item_index() { return (int64_t)blockIdx.x * kItemBlock + threadIdx.x; }

template <class Op>
inline void host_items(int64_t n, const Op& op) {
    for (int64_t i = 0; i < n; ++i) op(i);
}

// row i of (n, 8) rays, 16-byte aligned, by two 16-byte loads
__host__ __device__ inline void load_ray(const float4* __restrict__ rays, int64_t i, float* __restrict__ ray) {
    const float4 a = rays[2 * i], b = rays[2 * i + 1];
    ray[0] = a.x, ray[1] = a.y, ray[2] = a.z, ray[3] = a.w;
    ray[4] = b.x, ray[5] = b.y, ray[6] = b.z, ray[7] = b.w;
}

}  // namespace nerfhip
