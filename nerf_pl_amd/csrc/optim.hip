// N2: Adam on flat parameter storage — the reference's `Adam(lr, eps=1e-8, weight_decay)` over every
// parameter of both models (utils/__init__.py:10-30 -> torch.optim.Adam, non-amsgrad, L2 weight decay folded into the
// gradient), as ONE launch over up to 8 flat tensors instead of torch's multi-tensor apply (47 us for 1.19 M floats:
// launch/bookkeeping latency, not bandwidth — the update moves 4 x 4.8 MB).
//
//     t      = step + 1                                   (device-resident counter: hipGraph replays advance it)
//     g      = grad + weight_decay * param
//     m      = m + (g - m) (1 - beta1)                    (torch: exp_avg.lerp_(grad, 1 - beta1))
//     v      = beta2 v + (1 - beta2) g g
//     param -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
//
// HBM-bound: 16 B read + 12 B written per element, float4 per thread.  The step counter is advanced by the LAST
// workgroup to finish (arrival ticket), i.e. after every workgroup has read the old value.
//
// RAdam and Ranger (the reference's `--optimizer radam|ranger`: utils/optimizers.py:6-95 and :266-405, built by
// utils/__init__.py:21-26) on the same flat storage, the same table of up to 8 tensors and the same 2-float state.  Neither folds
// the weight decay into the gradient, and both put eps OUTSIDE the bias correction (torch.optim.RAdam does not: it is another
// optimizer).  With t = step + 1:
//
//     v      = beta2 v + (1 - beta2) g g ;   m = beta1 m + (1 - beta1) g                  (always, also when p stays put)
//     N_max  = 2 / (1 - beta2) - 1 ;         N_sma = N_max - 2 t beta2^t / (1 - beta2^t)
//     r      = sqrt((1 - beta2^t) (N_sma - 4) / (N_max - 4) (N_sma - 2) / N_sma N_max / (N_max - 2)) / (1 - beta1^t)
//
//   RAdam   N_sma >= 5           : p -= wd lr p ;  p -= r lr m / (sqrt(v) + eps)
//           else, degenerated    : p -= wd lr p ;  p -= lr / (1 - beta1^t) m
//           else                 : p untouched (no weight decay either)
//   Ranger  p -= wd lr p  always ;  N_sma > N_sma_threshhold : p -= r lr m / (sqrt(v) + eps)
//                                   else                     : p -= lr / (1 - beta1^t) m
//           then, when t % k == 0:  slow += alpha (p - slow) ;  p = slow
//           slow starts as the weights the FIRST step finds (the reference copies p.data inside its first step()): the t = 1
//           launch writes it before it updates p.  No other launch touches slow unless it is a sync step.
//
// N_sma, r and the products with lr are formed in DOUBLE, per thread, from double hyper-parameters, as the reference forms them
// in Python floats: with beta2 = 0.999, N_sma(5) = 4.99600 lies 0.004 under RAdam's threshold and fp32 loses that in the
// cancellation N_max - 2 t beta2^t / (1 - beta2^t) (4.986 at t = 5, 6.0005 for 5.9942 at t = 6), so the branch would be decided
// by rounding noise and r would be 0.16 % off through (N_sma - 4).  The coefficients are uniform over the launch, so the branches
// are too; the per-element arithmetic is fp32 on float4, as in adam_kernel.
#include "adam_math.h"

namespace nerfhip {

constexpr int kAdamMaxTensors = 8;
struct AdamTable {
    float* param[kAdamMaxTensors];
    const float* grad[kAdamMaxTensors];
    float* m[kAdamMaxTensors];
    float* v[kAdamMaxTensors];
    int64_t n[kAdamMaxTensors];
    int block0[kAdamMaxTensors + 1];   // first workgroup of each tensor
    int count;
};

constexpr int kAdamThreads = 256, kAdamVec = 4, kAdamPerBlock = kAdamThreads * kAdamVec * 4;   // 4096 floats / workgroup

// arrival ticket of the RAdam/Ranger kernels: the last workgroup advances the step counter (every workgroup read the old one
// before it got here).  adam_kernel keeps the same lines inline: moving them here reorders its instruction stream, and its
// measurements (profiles/) are of the stream it has.
__device__ __forceinline__ void advance_step(float* state, float t) {
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* ticket = reinterpret_cast<unsigned*>(state + 1);
        const unsigned prev = atomicAdd(ticket, 1u);
        if (prev == gridDim.x - 1) {
            *ticket = 0u;
            state[0] = t;
        }
    }
}

__global__ __launch_bounds__(kAdamThreads) void adam_kernel(AdamTable T, float* __restrict__ state, float lr, float beta1,
                                                            float beta2, float eps, float wd) {
    // state[0] = step count (float, exact up to 2^24 steps), state[1] (as unsigned) = arrival ticket
    const float t = state[0] + 1.0f;
    int ti = 0;
#pragma unroll
    for (int k = 1; k < kAdamMaxTensors; ++k) ti += (k < T.count && (int)blockIdx.x >= T.block0[k]) ? 1 : 0;
    const int64_t base = (int64_t)((int)blockIdx.x - T.block0[ti]) * kAdamPerBlock;
    const int64_t n = T.n[ti];
    float* __restrict__ P = T.param[ti];
    const float* __restrict__ G = T.grad[ti];
    float* __restrict__ M = T.m[ti];
    float* __restrict__ V = T.v[ti];
    const AdamCoef ac = adam_coef(t, lr, beta1, beta2);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = base + ((int64_t)r * kAdamThreads + threadIdx.x) * kAdamVec;
        if (i + kAdamVec <= n && ((((uintptr_t)(P + i)) | ((uintptr_t)(G + i)) | ((uintptr_t)(M + i)) | ((uintptr_t)(V + i))) & 15) == 0) {
            float4 p = *reinterpret_cast<const float4*>(P + i), g = *reinterpret_cast<const float4*>(G + i);
            float4 m = *reinterpret_cast<const float4*>(M + i), v = *reinterpret_cast<const float4*>(V + i);
            float* pp = &p.x; float* gp = &g.x; float* mp = &m.x; float* vp = &v.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) adam_elem(pp[k], gp[k], mp[k], vp[k], ac, beta2, eps, wd);
            *reinterpret_cast<float4*>(P + i) = p;
            *reinterpret_cast<float4*>(M + i) = m;
            *reinterpret_cast<float4*>(V + i) = v;
        } else {
            for (int k = 0; k < kAdamVec; ++k) {
                const int64_t j = i + k;
                if (j < n) adam_elem(P[j], G[j], M[j], V[j], ac, beta2, eps, wd);
            }
        }
    }
    // arrival ticket: the last workgroup advances the step counter (every workgroup read the old one above)
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* ticket = reinterpret_cast<unsigned*>(state + 1);
        const unsigned prev = atomicAdd(ticket, 1u);
        if (prev == gridDim.x - 1) {
            *ticket = 0u;
            state[0] = t;
        }
    }
}

struct SlowTable {
    float* slow[kAdamMaxTensors];      // Ranger's lookahead weights, one flat tensor per parameter tensor
};

// everything of one RAdam/Ranger launch that does not depend on the element
struct RadamCoef {
    float step_lr;      // -(step_size lr): rectified r, or 1 / (1 - beta1^t) in the degenerate form
    float wd_lr;        // -(weight_decay lr)
    float beta1, beta2, omb1, omb2, eps, alpha;
    int mode;           // 2: rectified, 1: degenerated to SGD with momentum, 0: moments only
    bool decay, sync, init;
};

template <bool kRanger>
__device__ __forceinline__ RadamCoef radam_coef(float t, double lr, double beta1, double beta2, double eps, double wd, double alpha,
                                                int k, double threshold, int degenerated_to_sgd) {
    RadamCoef c;
    const double td = (double)t;
    const double beta2_t = pow(beta2, td);
    const double n_max = 2.0 / (1.0 - beta2) - 1.0;
    const double n_sma = n_max - 2.0 * td * beta2_t / (1.0 - beta2_t);
    const double bc1 = 1.0 - pow(beta1, td);
    const bool rectified = kRanger ? (n_sma > threshold) : (n_sma >= threshold);
    double step_size;
    if (rectified) {
        step_size = sqrt((1.0 - beta2_t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) / bc1;
        c.mode = 2;
    } else {
        step_size = 1.0 / bc1;
        c.mode = (kRanger || degenerated_to_sgd) ? 1 : 0;
    }
    c.step_lr = (float)(-step_size * lr);
    c.wd_lr = (float)(-wd * lr);
    c.decay = wd != 0.0;
    c.beta1 = (float)beta1;
    c.beta2 = (float)beta2;
    c.omb1 = (float)(1.0 - beta1);
    c.omb2 = (float)(1.0 - beta2);
    c.eps = (float)eps;
    c.alpha = (float)alpha;
    c.sync = kRanger && ((int)t % k == 0);
    c.init = kRanger && t == 1.0f;
    return c;
}

// `s` is the element of the slow buffer: read by the caller only on sync steps, stored only when sync or init
template <bool kRanger>
__device__ __forceinline__ void radam_elem(float& p, float g, float& m, float& v, float& s, const RadamCoef& c) {
    v = v * c.beta2 + c.omb2 * g * g;
    m = m * c.beta1 + c.omb1 * g;
    if (c.mode == 0) return;
    float q = p;
    if (kRanger && c.init) s = q;
    if (c.decay) q = q + c.wd_lr * q;
    q = (c.mode == 2) ? q + c.step_lr * (m / (sqrtf(v) + c.eps)) : q + c.step_lr * m;
    if (kRanger && c.sync) {
        s = s + c.alpha * (q - s);
        q = s;
    }
    p = q;
}

template <bool kRanger>
__global__ __launch_bounds__(kAdamThreads) void radam_kernel(AdamTable T, SlowTable ST, float* __restrict__ state, double lr,
                                                             double beta1, double beta2, double eps, double wd, double alpha, int k,
                                                             double threshold, int degenerated_to_sgd) {
    const float t = state[0] + 1.0f;
    int ti = 0;
#pragma unroll
    for (int j = 1; j < kAdamMaxTensors; ++j) ti += (j < T.count && (int)blockIdx.x >= T.block0[j]) ? 1 : 0;
    const int64_t base = (int64_t)((int)blockIdx.x - T.block0[ti]) * kAdamPerBlock;
    const int64_t n = T.n[ti];
    float* __restrict__ P = T.param[ti];
    const float* __restrict__ G = T.grad[ti];
    float* __restrict__ M = T.m[ti];
    float* __restrict__ V = T.v[ti];
    const RadamCoef c = radam_coef<kRanger>(t, lr, beta1, beta2, eps, wd, alpha, k, threshold, degenerated_to_sgd);
    const bool slow_rd = kRanger && c.sync && !c.init, slow_wr = kRanger && (c.sync || c.init);     // uniform over the launch
    float* __restrict__ S = slow_wr ? ST.slow[ti] : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = base + ((int64_t)r * kAdamThreads + threadIdx.x) * kAdamVec;
        uintptr_t align = ((uintptr_t)(P + i)) | ((uintptr_t)(G + i)) | ((uintptr_t)(M + i)) | ((uintptr_t)(V + i));
        if (slow_wr) align |= (uintptr_t)(S + i);
        if (i + kAdamVec <= n && (align & 15) == 0) {
            float4 p = *reinterpret_cast<const float4*>(P + i), g = *reinterpret_cast<const float4*>(G + i);
            float4 m = *reinterpret_cast<const float4*>(M + i), v = *reinterpret_cast<const float4*>(V + i);
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            if (slow_rd) s = *reinterpret_cast<const float4*>(S + i);
            float* pp = &p.x; float* gp = &g.x; float* mp = &m.x; float* vp = &v.x; float* sp = &s.x;
#pragma unroll
            for (int e = 0; e < 4; ++e) radam_elem<kRanger>(pp[e], gp[e], mp[e], vp[e], sp[e], c);
            if (c.mode != 0) *reinterpret_cast<float4*>(P + i) = p;
            *reinterpret_cast<float4*>(M + i) = m;
            *reinterpret_cast<float4*>(V + i) = v;
            if (slow_wr) *reinterpret_cast<float4*>(S + i) = s;
        } else {
            for (int e = 0; e < kAdamVec; ++e) {
                const int64_t j = i + e;
                if (j < n) {
                    float p = P[j], m = M[j], v = V[j], s = slow_rd ? S[j] : 0.f;
                    radam_elem<kRanger>(p, G[j], m, v, s, c);
                    if (c.mode != 0) P[j] = p;
                    M[j] = m;
                    V[j] = v;
                    if (slow_wr) S[j] = s;
                }
            }
        }
    }
    advance_step(state, t);
}

}  // namespace nerfhip

namespace nerfhip {

// the launch table of `n_tensors` flat tensors and its workgroup count; NERFHIP_E_BADARG for what no launch may see
static int adam_table(AdamTable& T, int& blocks, float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                      float* const* exp_avg_sq_host, const int64_t* numel_host, int n_tensors) {
    NERFHIP_CHECK_ARG(params_host && grads_host && exp_avg_host && exp_avg_sq_host && numel_host);
    NERFHIP_CHECK_ARG(n_tensors >= 1 && n_tensors <= kAdamMaxTensors);
    blocks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        NERFHIP_CHECK_ARG(params_host[i] && grads_host[i] && exp_avg_host[i] && exp_avg_sq_host[i] && numel_host[i] > 0);
        T.param[i] = params_host[i];
        T.grad[i] = grads_host[i];
        T.m[i] = exp_avg_host[i];
        T.v[i] = exp_avg_sq_host[i];
        T.n[i] = numel_host[i];
        T.block0[i] = blocks;
        const int64_t nb = (numel_host[i] + kAdamPerBlock - 1) / kAdamPerBlock;
        if (nb + blocks > 0x3fffffff) return NERFHIP_E_BADARG;
        blocks += (int)nb;
    }
    for (int i = n_tensors; i < kAdamMaxTensors; ++i) {
        T.param[i] = nullptr; T.grad[i] = nullptr; T.m[i] = nullptr; T.v[i] = nullptr; T.n[i] = 0;
        T.block0[i] = blocks;
    }
    T.block0[kAdamMaxTensors] = blocks;
    T.count = n_tensors;
    return 0;
}

static bool radam_hyper_ok(double lr, double beta1, double beta2, double eps, double weight_decay) {
    return lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0;
}

}  // namespace nerfhip

extern "C" int nerfhip_adam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                                 float* const* exp_avg_sq_host, const int64_t* numel_host, int n_tensors, float* state,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(state);
    nerfhip::AdamTable T;
    int blocks = 0;
    const int rc = nerfhip::adam_table(T, blocks, params_host, grads_host, exp_avg_host, exp_avg_sq_host, numel_host, n_tensors);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(nerfhip::adam_kernel, dim3(blocks), dim3(nerfhip::kAdamThreads), 0, (hipStream_t)stream, T, state, lr,
                       beta1, beta2, eps, weight_decay);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_radam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                                  float* const* exp_avg_sq_host, const int64_t* numel_host, int n_tensors, float* state,
                                  double lr, double beta1, double beta2, double eps, double weight_decay, int degenerated_to_sgd,
                                  nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(state && nerfhip::radam_hyper_ok(lr, beta1, beta2, eps, weight_decay));
    nerfhip::AdamTable T;
    int blocks = 0;
    const int rc = nerfhip::adam_table(T, blocks, params_host, grads_host, exp_avg_host, exp_avg_sq_host, numel_host, n_tensors);
    if (rc != 0) return rc;
    nerfhip::SlowTable ST;
    for (int i = 0; i < nerfhip::kAdamMaxTensors; ++i) ST.slow[i] = nullptr;
    hipLaunchKernelGGL(nerfhip::radam_kernel<false>, dim3(blocks), dim3(nerfhip::kAdamThreads), 0, (hipStream_t)stream, T, ST, state,
                       lr, beta1, beta2, eps, weight_decay, 0.0, 1, 5.0, degenerated_to_sgd ? 1 : 0);
    return nerfhip_launch_status();
}

extern "C" int nerfhip_ranger_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                                   float* const* exp_avg_sq_host, const int64_t* numel_host, int n_tensors, float* state,
                                   float* const* slow_host, double alpha, int k, double n_sma_threshold, double lr, double beta1,
                                   double beta2, double eps, double weight_decay, nerfhip_stream_t stream) {
    NERFHIP_CHECK_ARG(state && slow_host && nerfhip::radam_hyper_ok(lr, beta1, beta2, eps, weight_decay));
    NERFHIP_CHECK_ARG(k >= 1 && alpha >= 0.0 && alpha <= 1.0);
    nerfhip::AdamTable T;
    int blocks = 0;
    const int rc = nerfhip::adam_table(T, blocks, params_host, grads_host, exp_avg_host, exp_avg_sq_host, numel_host, n_tensors);
    if (rc != 0) return rc;
    nerfhip::SlowTable ST;
    for (int i = 0; i < nerfhip::kAdamMaxTensors; ++i) {
        ST.slow[i] = i < n_tensors ? slow_host[i] : nullptr;
        NERFHIP_CHECK_ARG(i >= n_tensors || slow_host[i]);
    }
    hipLaunchKernelGGL(nerfhip::radam_kernel<true>, dim3(blocks), dim3(nerfhip::kAdamThreads), 0, (hipStream_t)stream, T, ST, state,
                       lr, beta1, beta2, eps, weight_decay, alpha, k, n_sma_threshold, 1);
    return nerfhip_launch_status();
}
