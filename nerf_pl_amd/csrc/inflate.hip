// Inflating a batch of zlib streams on the device (the IDAT data of a scene's PNG files), one workgroup of one wave per stream:
// blender.py:90 / llff.py's `Image.open(...)` without the host's zlib.  The wave alternates between the phases of inflate_core.h
// with a barrier between them; nothing is handed from wave to wave.  Back-references are read from the ring in LDS, never from
// bytes this launch stored; the ring leaves in 16-byte stores, 1 KiB per wave instruction.  nerfhip_inflate_host runs the same
// phase functions on the host, the 64 lanes in lockstep.
#include <new>

#include "common.h"
#include "inflate_core.h"

namespace {

using namespace nerfhip;
using namespace nerfhip::inflate;

struct Batch {
    const uint8_t* data;
    const int64_t* offsets;
    int64_t total_bytes;
    uint8_t* out;
    int64_t out_bytes, out_stride;
    int32_t* status;
};

NHI_HD Stream stream_of(const Batch& b, int i) {
    uint8_t* out = b.out + (int64_t)i * b.out_stride;
    return Stream{b.data + b.offsets[i], b.offsets[i + 1] - b.offsets[i], out, b.out_bytes, (int)((uintptr_t)out & 15)};
}

// The rounds of one stream: every round's decode_batch runs at least one step and a step consumes at least one bit, so there are
// at most 8 * nbytes + 2 rounds; the count below only keeps a broken invariant from spinning.
NHI_HD int64_t round_limit(const Stream& s) { return 8 * s.nbytes + 2; }

__global__ void __launch_bounds__(kLanes) inflate_streams(Batch b) {
    __shared__ Core c;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (check_stream(b.offsets, b.total_bytes, i) != 0) {            // (the whole workgroup)
        if (lane == 0) b.status[i] = NERFHIP_E_BADARG;
        return;
    }
    const Stream s = stream_of(b, i);
    init(c, lane);
    __syncthreads();
    for (int64_t round = 0, limit = round_limit(s); round < limit; ++round) {
        if (need_refill(c)) {
            __syncthreads();                             // (every lane has read bitpos and in_base)
            refill(c, s, lane);
        }
        __syncthreads();
        if (lane == 0) decode_batch(c, s);
        __syncthreads();
        place_literals(c, s, lane);
        __syncthreads();
        const int64_t base = s.mis + c.out_pos;
        for (int k = 0, n = c.nseq; k < n; ++k) {
            copy_token(c, s, base, k, lane);
            __syncthreads();
        }
        flush(c, s, lane);
        __syncthreads();
        if (lane == 0) after_flush(c, s);
        __syncthreads();
        if (c.finished) break;
        if (c.mode == kBuildFixed || c.mode == kBuildDynamic) {
            __syncthreads();                             // (every lane has read the mode before the last phase changes it)
            for (int phase = 0; phase < kBuildPhases; ++phase) {
                build_phase(c, phase, lane);
                __syncthreads();
            }
        }
    }
    if (lane == 0) b.status[i] = c.finished ? c.status : NERFHIP_E_DATA;
}

int check_args(const uint8_t* data, const int64_t* offsets, int64_t total_bytes, int n, uint8_t* out, int64_t out_bytes,
               int64_t out_stride, int32_t* status) {
    NERFHIP_CHECK_ARG(n >= 0 && n <= 65535 && total_bytes >= 0 && out_bytes >= 0 && out_stride >= out_bytes);
    if (n == 0) return 0;
    NERFHIP_CHECK_ARG(offsets && status && (data || total_bytes == 0) && (out || out_bytes == 0));
    NERFHIP_CHECK_ARG(out_bytes <= ((int64_t)1 << 40) && out_stride <= ((int64_t)1 << 40));
    if (((uintptr_t)offsets & 7) || ((uintptr_t)status & 3)) return NERFHIP_E_ALIGN;
    return 0;
}

}  // namespace

extern "C" int nerfhip_inflate(const uint8_t* data, const int64_t* offsets, int64_t total_bytes, int n_streams, uint8_t* out,
                               int64_t out_bytes, int64_t out_stride, int32_t* status, nerfhip_stream_t stream) {
    const int e = check_args(data, offsets, total_bytes, n_streams, out, out_bytes, out_stride, status);
    if (e || n_streams == 0) return e;
    const Batch b{data, offsets, total_bytes, out, out_bytes, out_stride, status};
    hipLaunchKernelGGL(inflate_streams, dim3((unsigned)n_streams), dim3(kLanes), 0, (hipStream_t)stream, b);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_inflate_host(const uint8_t* data, const int64_t* offsets, int64_t total_bytes, int n_streams, uint8_t* out,
                                    int64_t out_bytes, int64_t out_stride, int32_t* status) {
    const int e = check_args(data, offsets, total_bytes, n_streams, out, out_bytes, out_stride, status);
    if (e || n_streams == 0) return e;
    const Batch b{data, offsets, total_bytes, out, out_bytes, out_stride, status};
    Core* const core = new (std::nothrow) Core;
    if (!core) return NERFHIP_E_UNSUPPORTED;
    Core& c = *core;
    for (int i = 0; i < n_streams; ++i) {
        if (check_stream(offsets, total_bytes, i) != 0) {
            status[i] = NERFHIP_E_BADARG;
            continue;
        }
        const Stream s = stream_of(b, i);
        for (int lane = 0; lane < kLanes; ++lane) init(c, lane);
        for (int64_t round = 0, limit = round_limit(s); round < limit; ++round) {
            if (need_refill(c))
                for (int lane = 0; lane < kLanes; ++lane) refill(c, s, lane);
            decode_batch(c, s);
            for (int lane = 0; lane < kLanes; ++lane) place_literals(c, s, lane);
            for (int k = 0, n = c.nseq; k < n; ++k)
                for (int lane = 0; lane < kLanes; ++lane) copy_token(c, s, s.mis + c.out_pos, k, lane);
            for (int lane = 0; lane < kLanes; ++lane) flush(c, s, lane);
            after_flush(c, s);
            if (c.finished) break;
            if (c.mode == kBuildFixed || c.mode == kBuildDynamic)
                for (int phase = 0; phase < kBuildPhases; ++phase)
                    for (int lane = 0; lane < kLanes; ++lane) build_phase(c, phase, lane);
        }
        status[i] = c.finished ? c.status : NERFHIP_E_DATA;
    }
    delete core;
    return 0;
}
