// Epoch sampling on the device: every ray once per epoch, in the order of a keyed permutation (epoch_core.h).
// The reference trains on DataLoader(shuffle=True) (train.py:89-94): a fresh permutation of all n_images H W rays per epoch, the
// last batch partial.  Here the permutation is a function evaluated per position — no index tensor, no sort, no host work:
//
//   epoch_ids      one thread per id: the ids of positions [first, first + count) of a rank's share (host twin: epoch_ids_host)
//   epoch_batch    batch `cursor` of epoch `epoch` in ONE launch: permutation -> ray generation -> colour gather, by the device
//                  functions of nerfhip_sample_batch (rays_math.h gen_ray); epoch and cursor live in device memory and the last
//                  workgroup to finish advances them (the arrival ticket of draws_body.h), so a captured launch walks through the
//                  epochs on replay.
#include "epoch_core.h"
#include "rays_math.h"
#include "twin_launch.h"

namespace {

using nerfhip::blocks_of;
using nerfhip::EpochKey;

constexpr int kBlock = nerfhip::kItemBlock;
constexpr int64_t kMaxBatch = (int64_t)1 << 30;

__global__ void __launch_bounds__(kBlock) epoch_ids_kernel(EpochKey key, int64_t n, int rank, int world, int64_t first, int64_t count,
                                                           int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    out[i] = (int64_t)nerfhip::epoch_rank_id(key, n, rank, world, first + i);
}

struct EpochBatch {
    const float* c2w;
    const float* rgbs_all;
    float* rays;
    float* rgbs;
    int H, W;
    float focal, near, far;
    int use_ndc;
    float ndc_plane, sx, sy;
    int64_t n, B, share, steps;      // pixels; batch size; positions of this rank; batches per epoch
    int rank, world;
};

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// state = {seed, epoch, cursor, arrival ticket}.  Every workgroup reads (seed, epoch, cursor) first; the last one to finish
// writes the next (epoch, cursor).
__global__ void __launch_bounds__(kBlock) epoch_batch_kernel(EpochBatch a, unsigned long long* __restrict__ state,
                                                             int64_t* __restrict__ ids) {
    const unsigned long long seed = uniform64(state[0]), epoch = uniform64(state[1]);
    const unsigned long long cursor = uniform64(state[2]);
    const EpochKey key = nerfhip::epoch_key(seed, epoch);       // wave-uniform: expanded once, in scalar registers
    // a cursor outside the epoch (a state nobody should have written) serves no row and wraps below
    const int64_t start = cursor < (unsigned long long)a.steps ? (int64_t)cursor * a.B : a.share;
    const int64_t left = a.share - start;
    const int64_t rows = left < a.B ? left : a.B;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r < rows) {
        const int64_t id = (int64_t)nerfhip::epoch_rank_id(key, a.n, a.rank, a.world, start + r);
        if (ids) ids[r] = id;
        a.rgbs[3 * r] = a.rgbs_all[3 * id];
        a.rgbs[3 * r + 1] = a.rgbs_all[3 * id + 1];
        a.rgbs[3 * r + 2] = a.rgbs_all[3 * id + 2];
        nerfhip::gen_ray(a.c2w, id, a.H, a.W, a.focal, a.near, a.far, a.use_ndc, a.ndc_plane, a.sx, a.sy, a.rays + r * 8);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long prev = atomicAdd(state + 3, 1ull);
        if (prev == (unsigned long long)gridDim.x - 1ull) {
            const bool wrap = cursor + 1ull >= (unsigned long long)a.steps;
            state[3] = 0ull;
            state[2] = wrap ? 0ull : cursor + 1ull;
            state[1] = wrap ? epoch + 1ull : epoch;
        }
    }
}

// the checks every entry shares; *share = ceil(n / world)
inline int share_args(int64_t n, int rank, int world, int64_t* share) {
    NERFHIP_CHECK_ARG(n >= 1 && (uint64_t)n <= nerfhip::kEpochMaxN && world >= 1 && rank >= 0 && rank < world);
    *share = nerfhip::epoch_rank_share(n, world);
    return 0;
}

inline int ids_args(int64_t n, int rank, int world, int64_t first, int64_t count, const int64_t* out) {
    int64_t share = 0;
    const int e = share_args(n, rank, world, &share);
    if (e) return e;
    NERFHIP_CHECK_ARG(first >= 0 && count >= 0 && first <= share && count <= share - first);
    NERFHIP_CHECK_ARG(count == 0 || (out && (((uintptr_t)out) & 7) == 0));
    return 0;
}

}  // namespace

extern "C" int nerfhip_epoch_ids_host(uint64_t seed, uint64_t epoch, int64_t n, int rank, int world, int64_t first, int64_t count,
                                      int64_t* out) {
    const int e = ids_args(n, rank, world, first, count, out);
    if (e) return e;
    const EpochKey key = nerfhip::epoch_key(seed, epoch);
    for (int64_t i = 0; i < count; ++i) out[i] = (int64_t)nerfhip::epoch_rank_id(key, n, rank, world, first + i);
    return 0;
}

extern "C" int nerfhip_epoch_ids(uint64_t seed, uint64_t epoch, int64_t n, int rank, int world, int64_t first, int64_t count,
                                 int64_t* out_dev, nerfhip_stream_t stream) {
    const int e = ids_args(n, rank, world, first, count, out_dev);
    if (e || count == 0) return e;
    hipLaunchKernelGGL(epoch_ids_kernel, dim3(blocks_of(count)), dim3(kBlock), 0, (hipStream_t)stream, nerfhip::epoch_key(seed, epoch), n,
                       rank, world, first, count, out_dev);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_epoch_batch(const nerfhip_ray_batch* batch, int64_t n_pixels, int64_t B, int rank, int world, int drop_last,
                                   uint64_t* state, int64_t* ids_or_null, nerfhip_stream_t stream) {
    EpochBatch a;
    const int e = share_args(n_pixels, rank, world, &a.share);
    if (e) return e;
    // (a batch larger than the share is the DataLoader's one partial batch per epoch; dropping it would leave no batch at all)
    NERFHIP_CHECK_ARG(B >= 1 && B <= kMaxBatch && (!drop_last || B <= a.share) && batch && state);
    const nerfhip_ray_batch& b = *batch;
    NERFHIP_CHECK_ARG(b.c2w && b.rgbs_all && b.rays && b.rgbs && b.H > 0 && b.W > 0);
    NERFHIP_CHECK_ARG(((((uintptr_t)b.c2w) | ((uintptr_t)b.rgbs_all) | ((uintptr_t)b.rgbs)) & 3) == 0 && (((uintptr_t)b.rays) & 15) == 0);
    NERFHIP_CHECK_ARG(((((uintptr_t)state) | ((uintptr_t)ids_or_null)) & 7) == 0);
    a.c2w = b.c2w; a.rgbs_all = b.rgbs_all; a.rays = b.rays; a.rgbs = b.rgbs;
    a.H = b.H; a.W = b.W; a.focal = (float)b.focal; a.near = b.near; a.far = b.far;
    a.use_ndc = b.use_ndc; a.ndc_plane = b.ndc_near_plane;
    a.sx = nerfhip_ndc_scale(b.W, b.focal); a.sy = nerfhip_ndc_scale(b.H, b.focal);
    a.n = n_pixels; a.B = B; a.rank = rank; a.world = world;
    a.steps = drop_last ? a.share / B : (a.share + B - 1) / B;
    hipLaunchKernelGGL(epoch_batch_kernel, dim3(blocks_of(B)), dim3(kBlock), 0, (hipStream_t)stream, a,
                       reinterpret_cast<unsigned long long*>(state), ids_or_null);
    return nerfhip_launch_status();
}
