// SGD (momentum, Nesterov, weight decay) over ALL parameters of a group in ONE launch.
//
// The reference trains with torch.optim.SGD(nesterov=True) (core/builder.py:663-669, configs/nuscenes/default.yaml:18-23).
// On the device torch runs it as its multi-tensor ("foreach") path: five passes over parameters / gradients / momentum
// buffers in ~40 launches per step behind ~3.5 ms of host-side list handling (torch/optim/sgd.py:_multi_tensor_sgd) -- in a
// step that is bound by the host (NOTES N10).  Here: a job table (parameter, gradient, momentum buffer, elements, first-use
// flag per tensor) + one kernel that applies, element by element, the SAME five operations in the same order and with the same
// roundings as the foreach kernels (each `a + alpha * b` of ATen's BinaryOpListAlphaFunctor is one fused multiply-add; `b *
// momentum` and `b + g` round separately):
//     g1 = fma(wd, p, g)                      torch._foreach_add(grads, params, alpha=weight_decay)
//     b  = first ? g1 : (b * mom) + g1        clone(grad)  |  _foreach_mul_(bufs, momentum); _foreach_add_(bufs, grads, alpha=1)
//     g2 = nesterov ? fma(mom, b, g1) : b     _foreach_add_(grads, bufs, alpha=momentum)
//     p  = fma(-lr, g2, p)                    _foreach_add_(params, grads, alpha=-lr)
// bit-identical to torch's result (tests/test_gpu_optim.py), one read of p / g / b and one write of p / b per element.
//
// Under fp16 autocast a torch.amp.GradScaler stands in front of the step: unscale every gradient, look for a non-finite value,
// read the flag on the host, then step or not (torch/amp/grad_scaler.py) -- the launches and the wait that the one kernel
// above had removed.  Two more kernels over the SAME job table keep that on the device (optim.FusedSGD speaks the protocol of
// torch's fused optimizers, optim.GradScaler issues the check; tests/test_gpu_optim_amp.py, exact against torch):
//     grads_unscale_check_kernel   g *= *inv_scale (no store when it is 1), *found_inf = 1.0f where a product is not finite --
//                                  torch._amp_foreach_non_finite_check_and_unscale_ over all gradients of a group in one launch
//     sgd_batch_amp_kernel         the update above; *found_inf != 0: every workgroup returns before its first store;
//                                  grad_scale given: g = g * float(1.0 / double(*grad_scale)) first (GradScaler.unscale_'s
//                                  value and product), stored back to the gradient as torch's fused optimizers do
// (Stored values: torch's, element for element.  The flag is raised on the PRODUCT; torch raises it on the loaded value.  The two
// differ only for a finite gradient that overflows in the multiply -- an inverse scale above 1, a scale that has backed off
// below 1: such a step is skipped here, where torch would apply a gradient holding inf.)
// Both flags are plain floats that vector loads read and, for found_inf, vector stores of the one value 1.0f write.
#include "common.h"

namespace u2mkd {

constexpr int kSgdChunk = 4096;          // elements per workgroup (256 threads x 4 x float4)

struct SgdJob {                          // one row of the job table (int64 x 6)
    float *p;
    const float *g;                      // nullptr: this parameter received no gradient (skipped, as torch does)
    float *b;
    int64_t numel;
    int64_t first_chunk;                 // index of this tensor's first chunk in the launch
    int64_t first;                       // 1: no momentum buffer yet (torch: buf = clone(grad))
};

template <bool FMA>
__device__ __forceinline__ void sgd_one(float &p, float g, float &b, bool first, float lr_neg, float mom, float wd,
                                        bool use_wd, bool use_mom, bool nesterov) {
#pragma clang fp contract(off)
    float g1 = g;
    if (use_wd) g1 = FMA ? __builtin_fmaf(wd, p, g) : g + wd * p;
    float g2 = g1;
    if (use_mom) {
        float nb;
        if (first) {
            nb = g1;
        } else {
            nb = b * mom;
            nb = nb + g1;
        }
        b = nb;
        g2 = nesterov ? (FMA ? __builtin_fmaf(mom, nb, g1) : g1 + mom * nb) : nb;
    }
    p = FMA ? __builtin_fmaf(lr_neg, g2, p) : p + lr_neg * g2;
}

template <bool FMA>
__global__ void __launch_bounds__(256)
sgd_batch_kernel(const SgdJob *__restrict__ jobs, int n_jobs, float lr_neg, float mom, float wd, int use_wd, int use_mom,
                 int nesterov) {
    // which tensor owns this chunk: binary search over first_chunk (ascending)
    __shared__ int s_job;
    if (threadIdx.x == 0) {
        int lo = 0, hi = n_jobs - 1;
        const int64_t c = blockIdx.x;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
        }
        s_job = lo;
    }
    __syncthreads();
    const SgdJob j = jobs[s_job];
    if (j.g == nullptr) return;
    const int64_t base = ((int64_t)blockIdx.x - j.first_chunk) * kSgdChunk;
    if (base >= j.numel) return;
    const bool first = j.first != 0;
    const bool aligned = (((uintptr_t)j.p | (uintptr_t)j.g | (uintptr_t)j.b) & 15) == 0;
    const int64_t end = base + kSgdChunk < j.numel ? base + kSgdChunk : j.numel;
    if (aligned) {
        const int64_t end4 = base + ((end - base) & ~(int64_t)3);
        for (int64_t i = base + threadIdx.x * 4; i < end4; i += 256 * 4) {
            float4 p = *reinterpret_cast<const float4 *>(j.p + i);
            const float4 g = *reinterpret_cast<const float4 *>(j.g + i);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (use_mom && !first) b = *reinterpret_cast<const float4 *>(j.b + i);
            sgd_one<FMA>(p.x, g.x, b.x, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            sgd_one<FMA>(p.y, g.y, b.y, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            sgd_one<FMA>(p.z, g.z, b.z, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            sgd_one<FMA>(p.w, g.w, b.w, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            *reinterpret_cast<float4 *>(j.p + i) = p;
            if (use_mom) *reinterpret_cast<float4 *>(j.b + i) = b;
        }
        for (int64_t i = end4 + threadIdx.x; i < end; i += 256) {
            float p = j.p[i], b = (use_mom && !first) ? j.b[i] : 0.f;
            sgd_one<FMA>(p, j.g[i], b, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            j.p[i] = p;
            if (use_mom) j.b[i] = b;
        }
    } else {
        for (int64_t i = base + threadIdx.x; i < end; i += 256) {
            float p = j.p[i], b = (use_mom && !first) ? j.b[i] : 0.f;
            sgd_one<FMA>(p, j.g[i], b, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            j.p[i] = p;
            if (use_mom) j.b[i] = b;
        }
    }
}

// ---- the same update under a torch.amp.GradScaler: unscale, check and skip on the device -------------------------------------

__device__ __forceinline__ bool sgd_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ float sgd_unscale(float g, float inv) {
#pragma clang fp contract(off)
    return g * inv;
}

// which tensor owns this workgroup's chunk: binary search over first_chunk (ascending), as in sgd_batch_kernel
__device__ __forceinline__ SgdJob sgd_job_of_block(const SgdJob *__restrict__ jobs, int n_jobs) {
    __shared__ int s_job;
    if (threadIdx.x == 0) {
        int lo = 0, hi = n_jobs - 1;
        const int64_t c = blockIdx.x;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
        }
        s_job = lo;
    }
    __syncthreads();
    return jobs[s_job];
}

// g *= *inv_scale in place (nothing stored when it is 1), *found_inf = 1 where a product is not finite: the work of
// torch._amp_foreach_non_finite_check_and_unscale_ over all gradients of a group in one launch (it flags the loaded value;
// a non-finite value gives a non-finite product, so whatever torch flags is flagged here).
__global__ void __launch_bounds__(256)
grads_unscale_check_kernel(const SgdJob *__restrict__ jobs, int n_jobs, const float *__restrict__ inv_scale, float *found_inf) {
    const SgdJob j = sgd_job_of_block(jobs, n_jobs);
    if (j.g == nullptr) return;
    const int64_t base = ((int64_t)blockIdx.x - j.first_chunk) * kSgdChunk;
    if (base >= j.numel) return;
    const float inv = *inv_scale;
    const bool store = inv != 1.0f;
    float *g = const_cast<float *>(j.g);
    const int64_t end = base + kSgdChunk < j.numel ? base + kSgdChunk : j.numel;
    bool bad = false;
    int64_t scalar_from = base;
    if ((((uintptr_t)g) & 15) == 0) {
        const int64_t end4 = base + ((end - base) & ~(int64_t)3);
        for (int64_t i = base + threadIdx.x * 4; i < end4; i += 256 * 4) {
            float4 v = *reinterpret_cast<const float4 *>(g + i);
            v.x = sgd_unscale(v.x, inv); v.y = sgd_unscale(v.y, inv); v.z = sgd_unscale(v.z, inv); v.w = sgd_unscale(v.w, inv);
            bad |= !(sgd_finite(v.x) && sgd_finite(v.y) && sgd_finite(v.z) && sgd_finite(v.w));
            if (store) *reinterpret_cast<float4 *>(g + i) = v;
        }
        scalar_from = end4;
    }
    for (int64_t i = scalar_from + threadIdx.x; i < end; i += 256) {
        const float v = sgd_unscale(g[i], inv);
        bad |= !sgd_finite(v);
        if (store) g[i] = v;
    }
    if (bad) *found_inf = 1.0f;          // (the same value from any number of threads: a plain store, never cleared here)
}

// sgd_batch_kernel with the GradScaler's two device scalars: nothing is written when *found_inf != 0; with grad_scale every
// gradient is first multiplied by float(1 / double(*grad_scale)) -- GradScaler.unscale_'s value -- and stored back to .grad.
template <bool FMA>
__global__ void __launch_bounds__(256)
sgd_batch_amp_kernel(const SgdJob *__restrict__ jobs, int n_jobs, float lr_neg, float mom, float wd, int use_wd, int use_mom,
                     int nesterov, const float *__restrict__ grad_scale, const float *__restrict__ found_inf) {
    if (*found_inf != 0.f) return;       // (uniform over the launch: no workgroup stores anything)
    const SgdJob j = sgd_job_of_block(jobs, n_jobs);
    if (j.g == nullptr) return;
    const int64_t base = ((int64_t)blockIdx.x - j.first_chunk) * kSgdChunk;
    if (base >= j.numel) return;
    const bool unscale = grad_scale != nullptr;
    const float inv = unscale ? (float)(1.0 / (double)*grad_scale) : 1.0f;
    float *gw = const_cast<float *>(j.g);
    const bool first = j.first != 0;
    const bool aligned = (((uintptr_t)j.p | (uintptr_t)j.g | (uintptr_t)j.b) & 15) == 0;
    const int64_t end = base + kSgdChunk < j.numel ? base + kSgdChunk : j.numel;
    int64_t scalar_from = base;
    if (aligned) {
        const int64_t end4 = base + ((end - base) & ~(int64_t)3);
        for (int64_t i = base + threadIdx.x * 4; i < end4; i += 256 * 4) {
            float4 p = *reinterpret_cast<const float4 *>(j.p + i);
            float4 g = *reinterpret_cast<const float4 *>(j.g + i);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (use_mom && !first) b = *reinterpret_cast<const float4 *>(j.b + i);
            if (unscale) {
                g.x = sgd_unscale(g.x, inv); g.y = sgd_unscale(g.y, inv); g.z = sgd_unscale(g.z, inv); g.w = sgd_unscale(g.w, inv);
                *reinterpret_cast<float4 *>(gw + i) = g;
            }
            sgd_one<FMA>(p.x, g.x, b.x, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            sgd_one<FMA>(p.y, g.y, b.y, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            sgd_one<FMA>(p.z, g.z, b.z, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            sgd_one<FMA>(p.w, g.w, b.w, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
            *reinterpret_cast<float4 *>(j.p + i) = p;
            if (use_mom) *reinterpret_cast<float4 *>(j.b + i) = b;
        }
        scalar_from = end4;
    }
    for (int64_t i = scalar_from + threadIdx.x; i < end; i += 256) {
        float p = j.p[i], b = (use_mom && !first) ? j.b[i] : 0.f, g = j.g[i];
        if (unscale) {
            g = sgd_unscale(g, inv);
            gw[i] = g;
        }
        sgd_one<FMA>(p, g, b, first, lr_neg, mom, wd, use_wd, use_mom, nesterov);
        j.p[i] = p;
        if (use_mom) j.b[i] = b;
    }
}

}  // namespace u2mkd

using namespace u2mkd;

extern "C" {

int32_t u2mkd_sgd_chunk_elements(void) { return kSgdChunk; }

int u2mkd_sgd_batch(const int64_t *jobs, int32_t n_jobs, int64_t total_chunks, float lr, float momentum, float weight_decay,
                    int32_t nesterov, int32_t contract, u2mkd_stream_t s) {
    if (n_jobs == 0 || total_chunks == 0) return 0;
    U2_REQUIRE(jobs && n_jobs > 0 && total_chunks > 0 && total_chunks < (1LL << 31), "u2mkd_sgd_batch: bad job table");
    static_assert(sizeof(SgdJob) == 6 * sizeof(int64_t), "job table row = 6 x int64");
    const SgdJob *j = reinterpret_cast<const SgdJob *>(jobs);
    const float lr_neg = -lr;
    if (contract)
        hipLaunchKernelGGL(sgd_batch_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, as_stream(s), j, n_jobs, lr_neg,
                           momentum, weight_decay, weight_decay != 0.f, momentum != 0.f, nesterov);
    else
        hipLaunchKernelGGL(sgd_batch_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, as_stream(s), j, n_jobs, lr_neg,
                           momentum, weight_decay, weight_decay != 0.f, momentum != 0.f, nesterov);
    return check_launch("u2mkd_sgd_batch");
}

int u2mkd_grads_unscale_check(const int64_t *jobs, int32_t n_jobs, int64_t total_chunks, const float *inv_scale, float *found_inf,
                              u2mkd_stream_t s) {
    if (n_jobs == 0 || total_chunks == 0) return 0;
    U2_REQUIRE(jobs && n_jobs > 0 && total_chunks > 0 && total_chunks < (1LL << 31), "u2mkd_grads_unscale_check: bad job table");
    U2_REQUIRE(inv_scale && found_inf, "u2mkd_grads_unscale_check: inv_scale and found_inf are required");
    hipLaunchKernelGGL(grads_unscale_check_kernel, dim3((unsigned)total_chunks), dim3(256), 0, as_stream(s),
                       reinterpret_cast<const SgdJob *>(jobs), n_jobs, inv_scale, found_inf);
    return check_launch("u2mkd_grads_unscale_check");
}

int u2mkd_sgd_batch_amp(const int64_t *jobs, int32_t n_jobs, int64_t total_chunks, float lr, float momentum, float weight_decay,
                        int32_t nesterov, int32_t contract, const float *grad_scale, const float *found_inf, u2mkd_stream_t s) {
    if (n_jobs == 0 || total_chunks == 0) return 0;
    U2_REQUIRE(jobs && n_jobs > 0 && total_chunks > 0 && total_chunks < (1LL << 31), "u2mkd_sgd_batch_amp: bad job table");
    U2_REQUIRE(found_inf, "u2mkd_sgd_batch_amp: found_inf is required");
    const SgdJob *j = reinterpret_cast<const SgdJob *>(jobs);
    const float lr_neg = -lr;
    if (contract)
        hipLaunchKernelGGL(sgd_batch_amp_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, as_stream(s), j, n_jobs, lr_neg,
                           momentum, weight_decay, weight_decay != 0.f, momentum != 0.f, nesterov, grad_scale, found_inf);
    else
        hipLaunchKernelGGL(sgd_batch_amp_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, as_stream(s), j, n_jobs, lr_neg,
                           momentum, weight_decay, weight_decay != 0.f, momentum != 0.f, nesterov, grad_scale, found_inf);
    return check_launch("u2mkd_sgd_batch_amp");
}

}  // extern "C"
