// Shared by csrc/sptr.hip (one thread per (token, head)) and csrc/sptr_tiles.hip (16 x 16 tiles on the matrix pipe): the
// relative-position row of a (query, key) pair, sptr/modules.py:40-63 + spherical_transformer.py:39-64.
#pragma once
#include <stdlib.h>

#include "common.h"

namespace u2mkd {

constexpr int kHd = 16;        // head dim (asserted by the reference, sptr/functional.py:355)

// spherical_transformer.py:39-64 exponential_split on d = r_query - r_key
__device__ __forceinline__ int exp_split(float d, float a) {
    float da = fabsf(d);
    float flag = d >= 0.f ? 1.f : 0.f;
    float idx = 2.f * floorf(logf((da + 2.f * a) / a) / 0.6931471805599453f) - 2.f;
    float half = floorf(idx / 2.f);
    idx = idx + (((3.f * exp2f(half) - 2.f) * a <= da) ? 1.f : 0.f);
    idx = idx * (2.f * flag - 1.f) + (flag - 1.f);
    return (int)idx + 24;
}

// row strides (floats) of the token-major operands and the scale applied to q on load: lets the kernels read q, k, v
// straight out of the packed [N, 3, H, 16] output of the qkv projection (one branch = a range of heads), write the
// heads of a branch into their columns of the [N, H * 16] attention output, and the gradients into a packed
// [N, 3, H, 16] buffer -- without the slice / scale / concatenate copies around them
struct SptrLayout {
    int64_t ld_qkv, ld_out, ld_grad;
    float q_scale;
};

struct RelCtx {
    int qgl;        // quant_grid_length
    float a;        // > 0: spherical branch (exponential radial split + clamp)
};

__device__ __forceinline__ void rel_rows(const RelCtx &c, const int qi[3], float ri, const int qj[3], float rj,
                                         int r[3]) {
    r[0] = qi[0] - qj[0] + c.qgl - 1;
    r[1] = qi[1] - qj[1] + c.qgl - 1;
    r[2] = qi[2] - qj[2] + c.qgl - 1;
    if (c.a > 0.f) {
        r[2] = exp_split(ri - rj, c.a);
        const int hi = 2 * c.qgl - 1;
        r[0] = min(max(r[0], 0), hi);
        r[1] = min(max(r[1], 0), hi);
        r[2] = min(max(r[2], 0), hi);
    }
}

// ---- shared by csrc/sptr.hip and csrc/sptr_plain.hip ----------------------------------------------------------------
// the 16 channels of a (token, head) row, widened to fp32 (row types: common.h)
template <typename T>
__device__ __forceinline__ void load16(const T *p, float out[kHd]) {
    if constexpr (sizeof(T) == 2) p = static_cast<const T *>(__builtin_assume_aligned(p, 16));
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        float4 x = ld4<T>(p, v);
        out[4 * v] = x.x; out[4 * v + 1] = x.y; out[4 * v + 2] = x.z; out[4 * v + 3] = x.w;
    }
}

// ... and a row rounded to T once at its store
template <typename T>
__device__ __forceinline__ void store16(T *p, const float x[kHd]) {
    if constexpr (sizeof(T) == 2) p = static_cast<T *>(__builtin_assume_aligned(p, 16));
#pragma unroll
    for (int v = 0; v < 4; ++v) st4<T>(p, v, make_float4(x[4 * v], x[4 * v + 1], x[4 * v + 2], x[4 * v + 3]));
}

// delta[p,h] = sum_d dout[t,h,d] * out[t,h,d]
template <typename T>
__global__ void sptr_delta_kernel(const T *__restrict__ dout, const T *__restrict__ out,
                                  const int32_t *__restrict__ sort_idx, int64_t n, int h, float *__restrict__ delta,
                                  int64_t ld_out) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * h) return;
    int64_t p = e / h;
    int hh = (int)(e - p * h);
    int64_t t = sort_idx[p];
    float s = 0.f;
    if constexpr (sizeof(T) == 4) {
        const float *a = dout + t * ld_out + hh * kHd, *b = out + t * ld_out + hh * kHd;
#pragma unroll
        for (int d = 0; d < kHd; ++d) s += a[d] * b[d];
    } else {
        float a[kHd], b[kHd];
        load16(dout + t * ld_out + hh * kHd, a);
        load16(out + t * ld_out + hh * kHd, b);
#pragma unroll
        for (int d = 0; d < kHd; ++d) s += a[d] * b[d];
    }
    delta[e] = s;
}

// U2MKD_SPTR_SPLIT = 1 / 2 / 4 / 8 / 16: the lanes per (token, head) forced on every attention entry (read on every call); 0: not set
inline int sptr_forced_split() {
    const char *e = getenv("U2MKD_SPTR_SPLIT");
    const int forced = e ? atoi(e) : 0;
    return (forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 16) ? forced : 0;
}

}  // namespace u2mkd
