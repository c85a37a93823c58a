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
//
// Adam / AdamW (make_optimizer's `adam`, `adamw`, `adamw_spformer`: core/builder.py:670-718) the same way: u2mkd_adam_batch over a job
// table whose rows carry both moments (parameter, gradient, exp_avg, elements, first chunk, exp_avg_sq -- the check kernel above reads
// g / numel / first_chunk and serves it unchanged) applies, per element and in fp32, the operations of torch 2.10's
// _multi_tensor_adam (non-capturable) in torch's order:
//     p  = p * float(1 - lr wd)                 _foreach_mul_(params, 1 - lr * wd)          (decoupled: AdamW)
//     g  = fma(wd, p, g)                        _foreach_add(grads, params, alpha=wd)       (L2: Adam)
//     m  = lerp(m, g, float(1 - beta1))         _foreach_lerp_   |w| < 0.5: fma(w, g - m, m), else fma(-(g - m), 1 - w, g)
//     v  = v * float(beta2)                     _foreach_mul_
//     v  = fma(float(1 - beta2), g * g, v)      _foreach_addcmul_                           (g * g rounds first)
//     d  = sqrt(v) / bc2_sqrt + eps             _foreach_sqrt, _foreach_div_, _foreach_add_ (correctly rounded sqrt and division)
//     p  = fma(step_size, m / d, p)             _foreach_addcdiv_                           (correctly rounded division)
// Each spelling was settled stage by stage against the single torch._foreach_* call on gfx950 (tests/test_gpu_optim_adamw.py: every
// `a + s * x` is ONE fused multiply-add in torch's build, sqrt and both divisions are the correctly rounded ones) and is a launch
// argument (`form`), as `contract` is for SGD.  One read of p / g / m / v and one write of p / m / v per element.
// step_size = -lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come per job from a float table behind the job rows (one upload
// carries both), computed on the host in Python floats as torch computes them -- never a device pow.  Under a GradScaler
// (u2mkd_adam_batch_amp) a skipped step does not advance t, and only the device knows which steps were skipped: it keeps a count of
// applied steps in two int32 slots (call n reads slot n & 1; one thread of the step's last launch stores the other slot, a plain C++
// store), the host sends each job's scalars for every count the device could be at (`window` rows) and the kernel takes row
// `count - count_known`.  *found_inf != 0: every workgroup returns before its first store to a parameter, a moment or a gradient.
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

// ---- Adam / AdamW over all parameters of a group in one launch (see the header comment) --------------------------------------

struct AdamJob {                         // one row of the job table (int64 x 6): SgdJob's layout with the second moment in its last column
    float *p;
    const float *g;                      // nullptr: this parameter received no gradient (skipped, as torch does)
    float *m;                            // exp_avg
    int64_t numel;
    int64_t first_chunk;
    float *v;                            // exp_avg_sq
};
static_assert(sizeof(AdamJob) == sizeof(SgdJob), "one job table serves the check kernel and both updates");

struct AdamK {                           // the group's scalars, each rounded to fp32 once on the host (as ATen takes a Scalar)
    float decay;                         // float(1 - lr * wd)      (decoupled)
    float wd;                            //                          (L2)
    float w1;                            // float(1 - beta1)
    float beta2;
    float w2;                            // float(1 - beta2)
    float eps;
    int mode;                            // 0: no weight decay, 1: decoupled (AdamW), 2: L2 (Adam)
    int form;                            // kAdam* bits below
};

// which of two spellings each stage takes (a launch argument, as `contract` is for SGD; settled by tests/test_gpu_optim_adamw.py's
// stage probes against the single torch._foreach_* call)
constexpr int kAdamFmaL2 = 1, kAdamFmaLerp = 2, kAdamFmaAddcmul = 4, kAdamFmaAddcdiv = 8;
constexpr int kAdamSqrtShift = 4, kAdamDivScalarShift = 6, kAdamDivShift = 8;      // 2 bits each: 0 correctly rounded, 1 / 2 below

__device__ __forceinline__ float adam_lerp(float m, float g, float w, int form) {
#pragma clang fp contract(off)
    const float diff = g - m;            // ATen/native/Lerp.h
    if (__builtin_fabsf(w) < 0.5f) return (form & kAdamFmaLerp) ? __builtin_fmaf(w, diff, m) : m + w * diff;
    const float r = 1.0f - w;
    return (form & kAdamFmaLerp) ? __builtin_fmaf(-diff, r, g) : g - diff * r;
}

__device__ __forceinline__ float adam_addcmul(float v, float a, float b, float s, int form) {
#pragma clang fp contract(off)
    const float ab = a * b;              // (rounds first: ForeachFunctors.cuh, pointwise_op_scalar)
    return (form & kAdamFmaAddcmul) ? __builtin_fmaf(s, ab, v) : v + s * ab;
}

__device__ __forceinline__ float adam_sqrt(float v, int how) {
#pragma clang fp contract(off)
    return how == 1 ? __builtin_amdgcn_sqrtf(v) : __builtin_sqrtf(v);
}

__device__ __forceinline__ float adam_div(float a, float b, int how) {
#pragma clang fp contract(off)
    if (how == 1) return a * (1.0f / b);
    if (how == 2) return a * __builtin_amdgcn_rcpf(b);
    return a / b;
}

__device__ __forceinline__ float adam_addcdiv(float p, float m, float d, float s, int form) {
#pragma clang fp contract(off)
    const float q = adam_div(m, d, (form >> kAdamDivShift) & 3);
    return (form & kAdamFmaAddcdiv) ? __builtin_fmaf(s, q, p) : p + s * q;
}

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const AdamK &k, float step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
    if (k.mode == 1) p = p * k.decay;
    else if (k.mode == 2) g = (k.form & kAdamFmaL2) ? __builtin_fmaf(k.wd, p, g) : g + k.wd * p;
    m = adam_lerp(m, g, k.w1, k.form);
    v = v * k.beta2;
    v = adam_addcmul(v, g, g, k.w2, k.form);
    float d = adam_sqrt(v, (k.form >> kAdamSqrtShift) & 3);
    d = adam_div(d, bc2_sqrt, (k.form >> kAdamDivScalarShift) & 3);
    d = d + k.eps;
    p = adam_addcdiv(p, m, d, step_size, k.form);
}

// AMP: the GradScaler's two device scalars and the device's count of applied steps (see u2mkd_adam_batch_amp in the header)
template <bool AMP>
__global__ void __launch_bounds__(256)
adam_batch_kernel(const AdamJob *__restrict__ jobs, int n_jobs, const float *__restrict__ scalars, AdamK k, int window,
                  const int32_t *__restrict__ count_in, int32_t *count_out, int32_t count_known,
                  const float *__restrict__ grad_scale, const float *__restrict__ found_inf) {
    int row = 0;
    if (AMP) {
        const bool skip = *found_inf != 0.f;
        const int32_t applied = count_in ? *count_in : 0;
        if (count_out && blockIdx.x == 0 && threadIdx.x == 0) *count_out = applied + (skip ? 0 : 1);      // (a plain store by one thread)
        if (skip) return;                // (uniform over the launch: no workgroup stores a parameter, a moment or a gradient)
        if (count_in) {
            row = applied - count_known;
            row = row < 0 ? 0 : (row >= window ? window - 1 : row);      // (never past the table, whatever the host believed)
        }
    }
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
    const int ji = s_job;
    const AdamJob j = jobs[ji];
    if (j.g == nullptr) return;
    const int64_t base = ((int64_t)blockIdx.x - j.first_chunk) * kSgdChunk;
    if (base >= j.numel) return;
    const float step_size = scalars[((int64_t)ji * window + row) * 2], bc2_sqrt = scalars[((int64_t)ji * window + row) * 2 + 1];
    const bool unscale = AMP && grad_scale != nullptr;
    const float inv = unscale ? (float)(1.0 / (double)*grad_scale) : 1.0f;
    float *gw = const_cast<float *>(j.g);
    const bool aligned = (((uintptr_t)j.p | (uintptr_t)j.g | (uintptr_t)j.m | (uintptr_t)j.v) & 15) == 0;
    const int64_t end = base + kSgdChunk < j.numel ? base + kSgdChunk : j.numel;
    int64_t scalar_from = base;
    if (aligned) {
        const int64_t end4 = base + ((end - base) & ~(int64_t)3);
        for (int64_t i = base + threadIdx.x * 4; i < end4; i += 256 * 4) {
            float4 p = *reinterpret_cast<const float4 *>(j.p + i);
            float4 g = *reinterpret_cast<const float4 *>(j.g + i);
            float4 m = *reinterpret_cast<const float4 *>(j.m + i);
            float4 v = *reinterpret_cast<const float4 *>(j.v + i);
            if (unscale) {
                g.x = sgd_unscale(g.x, inv); g.y = sgd_unscale(g.y, inv); g.z = sgd_unscale(g.z, inv); g.w = sgd_unscale(g.w, inv);
                *reinterpret_cast<float4 *>(gw + i) = g;
            }
            adam_one(p.x, g.x, m.x, v.x, k, step_size, bc2_sqrt);
            adam_one(p.y, g.y, m.y, v.y, k, step_size, bc2_sqrt);
            adam_one(p.z, g.z, m.z, v.z, k, step_size, bc2_sqrt);
            adam_one(p.w, g.w, m.w, v.w, k, step_size, bc2_sqrt);
            *reinterpret_cast<float4 *>(j.p + i) = p;
            *reinterpret_cast<float4 *>(j.m + i) = m;
            *reinterpret_cast<float4 *>(j.v + i) = v;
        }
        scalar_from = end4;
    }
    for (int64_t i = scalar_from + threadIdx.x; i < end; i += 256) {
        float p = j.p[i], g = j.g[i], m = j.m[i], v = j.v[i];
        if (unscale) {
            g = sgd_unscale(g, inv);
            gw[i] = g;
        }
        adam_one(p, g, m, v, k, step_size, bc2_sqrt);
        j.p[i] = p;
        j.m[i] = m;
        j.v[i] = v;
    }
}

// one stage of adam_one over n elements (the stage probes: each against the single torch._foreach_* call it restates)
__global__ void __launch_bounds__(256)
adam_stage_kernel(int stage, int form, const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c,
                  float s, float *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float r = 0.f;
    switch (stage) {
        case 0: r = adam_lerp(a[i], b[i], s, form); break;
        case 1: r = adam_addcmul(a[i], b[i], c[i], s, form); break;
        case 2: r = adam_sqrt(a[i], (form >> kAdamSqrtShift) & 3); break;
        case 3: r = adam_div(a[i], s, (form >> kAdamDivScalarShift) & 3); break;
        case 4: r = adam_addcdiv(a[i], b[i], c[i], s, form); break;
        default: break;
    }
    out[i] = r;
}

}  // namespace u2mkd

using namespace u2mkd;

extern "C" {

static AdamK adam_k(float decay, float weight_decay, int32_t decoupled, float w1, float beta2, float w2, float eps, int32_t form) {
    AdamK k;
    k.decay = decay; k.wd = weight_decay; k.w1 = w1; k.beta2 = beta2; k.w2 = w2; k.eps = eps;
    k.mode = weight_decay == 0.f ? 0 : (decoupled ? 1 : 2);
    k.form = form;
    return k;
}

int u2mkd_adam_batch(const int64_t *jobs, int32_t n_jobs, int64_t total_chunks, const float *scalars, float decay, float weight_decay,
                     int32_t decoupled, float w1, float beta2, float w2, float eps, int32_t form, u2mkd_stream_t s) {
    if (n_jobs == 0 || total_chunks == 0) return 0;
    U2_REQUIRE(jobs && scalars && n_jobs > 0 && total_chunks > 0 && total_chunks < (1LL << 31), "u2mkd_adam_batch: bad job table");
    hipLaunchKernelGGL(adam_batch_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, as_stream(s),
                       reinterpret_cast<const AdamJob *>(jobs), n_jobs, scalars, adam_k(decay, weight_decay, decoupled, w1, beta2, w2, eps, form),
                       1, (const int32_t *)nullptr, (int32_t *)nullptr, 0, (const float *)nullptr, (const float *)nullptr);
    return check_launch("u2mkd_adam_batch");
}

int u2mkd_adam_batch_amp(const int64_t *jobs, int32_t n_jobs, int64_t total_chunks, const float *scalars, int32_t window, float decay,
                         float weight_decay, int32_t decoupled, float w1, float beta2, float w2, float eps, int32_t form,
                         const int32_t *count_in, int32_t *count_out, int32_t count_known, const float *grad_scale,
                         const float *found_inf, u2mkd_stream_t s) {
    if (n_jobs == 0 || total_chunks == 0) return 0;
    U2_REQUIRE(jobs && scalars && n_jobs > 0 && total_chunks > 0 && total_chunks < (1LL << 31), "u2mkd_adam_batch_amp: bad job table");
    U2_REQUIRE(found_inf, "u2mkd_adam_batch_amp: found_inf is required");
    U2_REQUIRE(window >= 1 && (count_in || window == 1), "u2mkd_adam_batch_amp: a window above 1 needs the device's count");
    U2_REQUIRE(count_in != count_out || !count_out, "u2mkd_adam_batch_amp: count_in and count_out are two slots");
    hipLaunchKernelGGL(adam_batch_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, as_stream(s),
                       reinterpret_cast<const AdamJob *>(jobs), n_jobs, scalars, adam_k(decay, weight_decay, decoupled, w1, beta2, w2, eps, form),
                       window, count_in, count_out, count_known, grad_scale, found_inf);
    return check_launch("u2mkd_adam_batch_amp");
}

int u2mkd_debug_adam_stage(int32_t stage, int32_t form, const float *a, const float *b, const float *c, float scalar, float *out,
                           int64_t n, u2mkd_stream_t s) {
    if (n == 0) return 0;
    U2_REQUIRE(stage >= 0 && stage <= 4 && a && out && n > 0 && n < (1LL << 39), "u2mkd_debug_adam_stage: bad arguments");
    U2_REQUIRE((stage != 0 && stage != 1 && stage != 4) || b, "u2mkd_debug_adam_stage: this stage reads b");
    U2_REQUIRE((stage != 1 && stage != 4) || c, "u2mkd_debug_adam_stage: this stage reads c");
    hipLaunchKernelGGL(adam_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(s), stage, form, a, b, c, scalar, out, n);
    return check_launch("u2mkd_debug_adam_stage");
}

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
