// LayerNorm over the rows of a [N, C] feature matrix, optionally fused with the residual add in front of it.
// Replaces nn.LayerNorm (norm1, norm2) of the SphereFormer block (spherical_transformer.py:316-348; SURVEY.md section 8a
// row a10) and, in the add form, the residual sum `short_cut + drop_path(attn)` that feeds norm2.
//
// HBM-bound row work, one pass per direction:
//   forward   a lane group of G lanes (8..64, chosen from C) owns a row: 8 channels per lane and chunk, 16-byte loads, the
//             row stays in registers between the statistics and the normalise step.  mean = sum / C, then the variance from
//             the squared deviations OF THOSE REGISTERS (never E[x^2] - mean^2), both reduced inside the lane group with
//             cross-lane adds (xor butterfly: every lane of the group ends with the same bits).  No LDS.
//             add form: s = a + w_r * b (one fp32 fma, rounded ONCE to the row type), s is stored as the new residual-stream
//             row and the statistics are taken from the ROUNDED s, so y == LN(stored s) bit for bit.
//   backward  dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dy * gamma [+ ds] [, db = w_r * dx_total] in one
//             pass; dgamma / dbeta accumulate in registers over the workgroup's slab of rows, are combined across the lane
//             groups of a wave with cross-lane adds, across the four waves through LDS in wave order, and leave as one
//             partial [2, C] per slab.  A second small kernel sums the slabs in a fixed order.  No atomics; the slab
//             partition depends on n alone, so the sums are the same bits on every device and in every run.
// ARITHMETIC.  Rows, parameters, saved statistics, the register accumulators of dgamma / dbeta and the slab partials are fp32;
// the arithmetic BETWEEN a load and a store -- a row's sums, mean, variance and 1 / sqrt, the normalise expression, the dx
// expression, the cross-lane sum of the accumulators and the slab sum -- is carried in double and rounded once.  In fp32 an element
// of y or dx passes three to five roundings; at n = 1 that put single outputs 1.1 to 1.8 units in the last place off where torch's
// kernels happened to be 0.4 to 0.8 off (7 of 1 260 cases of tests/test_gpu_row_layernorm.py), more than the factor two that
// test allows.  The kernels move 16 to 64 bytes per lane and row and are bound by memory; not timed (NOTES N17.5).  A 16-bit value
// is widened exactly on load and rounded to nearest even at its store.
#include "common.h"

#include <initializer_list>

namespace u2mkd {

constexpr int kLnThreads = 256;
constexpr int kLnFwdRows = 32;     // rows per workgroup in the forward (one trip of the 8-lane form, eight of the 64-lane form)
constexpr int kLnSlabRows = 128;   // rows per workgroup (= per dgamma / dbeta partial) in the backward
constexpr int kLnFinLanes = 64, kLnFinItems = 4;

// 8 consecutive channels of a row (index in units of 8 elements): one 16-byte access for 16-bit rows, two for fp32
struct f8 { float v[8]; };
typedef _Float16 u2_f16row8 __attribute__((ext_vector_type(8)));

template <typename T> __device__ __forceinline__ f8 ld8(const T *p, int64_t i8);
template <> __device__ __forceinline__ f8 ld8<float>(const float *p, int64_t i8) {
    const float4 a = reinterpret_cast<const float4 *>(p)[2 * i8], b = reinterpret_cast<const float4 *>(p)[2 * i8 + 1];
    return f8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
template <> __device__ __forceinline__ f8 ld8<bf16row>(const bf16row *p, int64_t i8) {
    const uint4 w = reinterpret_cast<const uint4 *>(p)[i8];     // a bf16 is the upper half of the fp32 with the same value
    return f8{{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
               __uint_as_float(w.y & 0xffff0000u), __uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u),
               __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)}};
}
template <> __device__ __forceinline__ f8 ld8<_Float16>(const _Float16 *p, int64_t i8) {
    const u2_f16row8 h = reinterpret_cast<const u2_f16row8 *>(p)[i8];
    return f8{{(float)h[0], (float)h[1], (float)h[2], (float)h[3], (float)h[4], (float)h[5], (float)h[6], (float)h[7]}};
}

__device__ __forceinline__ uint32_t ln_bf16_pair(float lo, float hi) {
    const __bf16 a = (__bf16)lo, b = (__bf16)hi;      // round to nearest even, NaN stays NaN
    return (uint32_t)__builtin_bit_cast(unsigned short, a) | ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
}
template <typename T> __device__ __forceinline__ void st8(T *p, int64_t i8, const f8 &o);
template <> __device__ __forceinline__ void st8<float>(float *p, int64_t i8, const f8 &o) {
    reinterpret_cast<float4 *>(p)[2 * i8] = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
    reinterpret_cast<float4 *>(p)[2 * i8 + 1] = make_float4(o.v[4], o.v[5], o.v[6], o.v[7]);
}
template <> __device__ __forceinline__ void st8<bf16row>(bf16row *p, int64_t i8, const f8 &o) {
    uint4 w;
    w.x = ln_bf16_pair(o.v[0], o.v[1]); w.y = ln_bf16_pair(o.v[2], o.v[3]);
    w.z = ln_bf16_pair(o.v[4], o.v[5]); w.w = ln_bf16_pair(o.v[6], o.v[7]);
    reinterpret_cast<uint4 *>(p)[i8] = w;
}
template <> __device__ __forceinline__ void st8<_Float16>(_Float16 *p, int64_t i8, const f8 &o) {
    const u2_f16row8 h = {(_Float16)o.v[0], (_Float16)o.v[1], (_Float16)o.v[2], (_Float16)o.v[3],
                          (_Float16)o.v[4], (_Float16)o.v[5], (_Float16)o.v[6], (_Float16)o.v[7]};      // overflow -> inf
    reinterpret_cast<u2_f16row8 *>(p)[i8] = h;
}

// the value a store of the row type leaves behind, as fp32
template <typename T> __device__ __forceinline__ float ln_round(float v);
template <> __device__ __forceinline__ float ln_round<float>(float v) { return v; }
template <> __device__ __forceinline__ float ln_round<bf16row>(float v) { return (float)(__bf16)v; }
template <> __device__ __forceinline__ float ln_round<_Float16>(float v) { return (float)(_Float16)v; }

// sum over the G lanes of a lane group (G a power of two, groups aligned): xor butterfly, the same bits in every lane
template <int G>
__device__ __forceinline__ double ln_group_sum(double v) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// G lanes per row, V chunks of 8 channels per lane (G * V * 8 >= C; V = 2 only for C > 512)
// ADD: s = a + w_r * b (w may be null: a + b), s_out = s rounded to T, y = LN(s_out); else y = LN(a)
template <typename T, int G, int V, bool ADD>
__global__ void __launch_bounds__(kLnThreads)
ln_fwd_kernel(const T *__restrict__ a, const T *__restrict__ b, const float *__restrict__ w, int64_t n, int c,
              const float *__restrict__ gamma, const float *__restrict__ beta, float eps, T *__restrict__ s_out,
              T *__restrict__ y, float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    constexpr int kRows = kLnThreads / G;      // rows per trip
    const int c8 = c >> 3;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    f8 gm[V], bt[V];
    bool on[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
        const int ch = lane + u * G;
        on[u] = ch < c8;
        if (on[u]) {
            gm[u] = ld8<float>(gamma, ch);
            bt[u] = ld8<float>(beta, ch);
        } else {
            gm[u] = f8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
            bt[u] = gm[u];
        }
    }
    const double inv_c = 1.0 / (double)c;
    const int64_t r0 = (int64_t)blockIdx.x * kLnFwdRows;
#pragma unroll 1
    for (int t = 0; t < kLnFwdRows / kRows; ++t) {
        const int64_t r = r0 + t * kRows + grp;
        const bool live = r < n;      // (a dead row's lanes still take part in the cross-lane sums, with zeros)
        f8 v[V];
        double sum = 0.0;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const bool ok = live && on[u];
            const int64_t i8 = r * c8 + lane + u * G;
            v[u] = ok ? ld8<T>(a, i8) : f8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
            if (ADD) {
                if (ok) {
                    const f8 q = ld8<T>(b, i8);
                    const float wr = w ? w[r] : 1.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[u].v[k] = ln_round<T>(__fmaf_rn(wr, q.v[k], v[u].v[k]));
                    st8<T>(s_out, i8, v[u]);
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += (double)v[u].v[k];
        }
        // the statistics of a row and the normalise step are carried in double and every stored value is rounded once: a row of
        // one repeated value has that value as its mean exactly (variance 0, y = beta), and an element of y is half a unit in the
        // last place from what its row's exact statistics give
        const double mean = ln_group_sum<G>(sum) * inv_c;
        double m2 = 0.0;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (on[u]) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const double d = (double)v[u].v[k] - mean;
                    m2 += d * d;
                }
            }
        }
        const double rstd = 1.0 / sqrt(ln_group_sum<G>(m2) * inv_c + (double)eps);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (live && on[u]) {
                f8 o;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    o.v[k] = (float)(((double)v[u].v[k] - mean) * rstd * (double)gm[u].v[k] + (double)bt[u].v[k]);
                st8<T>(y, r * c8 + lane + u * G, o);
            }
        }
        if (live && lane == 0 && mean_out) {
            mean_out[r] = (float)mean;
            rstd_out[r] = (float)rstd;
        }
    }
}

// dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) [+ ds], db = w_r * dx (when db is given);
// partial [slab][2][c] = (sum_rows dy * xhat, sum_rows dy) over the slab's rows
template <typename T, int G, int V>
__global__ void __launch_bounds__(kLnThreads)
ln_bwd_kernel(const T *__restrict__ dy, const T *__restrict__ x, const T *__restrict__ ds, const float *__restrict__ w,
              int64_t n, int c, const float *__restrict__ mean, const float *__restrict__ rstd,
              const float *__restrict__ gamma, T *__restrict__ dx, T *__restrict__ db, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float red[];      // [4 waves][2][c]
    constexpr int kRows = kLnThreads / G;
    const int c8 = c >> 3;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    f8 gm[V], dg[V], dbt[V];
    bool on[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
        const int ch = lane + u * G;
        on[u] = ch < c8;
        dg[u] = f8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
        dbt[u] = dg[u];
        gm[u] = on[u] ? ld8<float>(gamma, ch) : dg[u];
    }
    const double inv_c = 1.0 / (double)c;
    const int64_t r0 = (int64_t)blockIdx.x * kLnSlabRows;
#pragma unroll 1
    for (int t = 0; t < kLnSlabRows / kRows; ++t) {
        const int64_t r = r0 + t * kRows + grp;
        const bool live = r < n;
        const double mu = live ? (double)mean[r] : 0.0, rs = live ? (double)rstd[r] : 0.0;
        f8 d[V], xv[V];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const bool ok = live && on[u];
            const int64_t i8 = r * c8 + lane + u * G;
            const f8 zero = f8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
            d[u] = ok ? ld8<T>(dy, i8) : zero;
            xv[u] = ok ? ld8<T>(x, i8) : zero;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double h = ok ? ((double)xv[u].v[k] - mu) * rs : 0.0;
                const double g = (double)d[u].v[k] * (double)gm[u].v[k];
                s1 += g;
                s2 += g * h;
                dg[u].v[k] += (float)((double)d[u].v[k] * h);      // (rows of the slab in trip order: a fixed order)
                dbt[u].v[k] += d[u].v[k];
            }
        }
        s1 = ln_group_sum<G>(s1) * inv_c;
        s2 = ln_group_sum<G>(s2) * inv_c;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (live && on[u]) {
                const int64_t i8 = r * c8 + lane + u * G;
                f8 e = f8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
                if (ds) e = ld8<T>(ds, i8);
                f8 o;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const double h = ((double)xv[u].v[k] - mu) * rs;
                    const double g = (double)d[u].v[k] * (double)gm[u].v[k];
                    o.v[k] = (float)(rs * (g - s1 - h * s2) + (double)e.v[k]);      // (one rounding, the arriving gradient included)
                }
                st8<T>(dx, i8, o);
                if (db) {
                    const float wr = w[r];
#pragma unroll
                    for (int k = 0; k < 8; ++k) o.v[k] *= wr;
                    st8<T>(db, i8, o);
                }
            }
        }
    }
    // the lane groups of a wave (cross-lane, in double, rounded once), then the four waves (LDS, wave order)
    const int wl = threadIdx.x % kWave, wv = threadIdx.x / kWave;
#pragma unroll
    for (int u = 0; u < V; ++u) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double a = (double)dg[u].v[k], b = (double)dbt[u].v[k];
#pragma unroll
            for (int o = G; o < kWave; o <<= 1) {
                a += __shfl_xor(a, o);
                b += __shfl_xor(b, o);
            }
            dg[u].v[k] = (float)a;
            dbt[u].v[k] = (float)b;
        }
        if (wl < G && on[u]) {
            float *p = red + (size_t)wv * 2 * c + 8 * (lane + u * G);
            *reinterpret_cast<float4 *>(p) = make_float4(dg[u].v[0], dg[u].v[1], dg[u].v[2], dg[u].v[3]);
            *reinterpret_cast<float4 *>(p + 4) = make_float4(dg[u].v[4], dg[u].v[5], dg[u].v[6], dg[u].v[7]);
            *reinterpret_cast<float4 *>(p + c) = make_float4(dbt[u].v[0], dbt[u].v[1], dbt[u].v[2], dbt[u].v[3]);
            *reinterpret_cast<float4 *>(p + c + 4) = make_float4(dbt[u].v[4], dbt[u].v[5], dbt[u].v[6], dbt[u].v[7]);
        }
    }
    __syncthreads();
    const int n4 = c >> 1;      // float4s of one [2][c] partial
    for (int i = threadIdx.x; i < n4; i += kLnThreads) {
        float4 t = reinterpret_cast<const float4 *>(red)[i];
#pragma unroll
        for (int q = 1; q < kLnThreads / kWave; ++q) {
            const float4 e = reinterpret_cast<const float4 *>(red + (size_t)q * 2 * c)[i];
            t.x += e.x; t.y += e.y; t.z += e.z; t.w += e.w;
        }
        reinterpret_cast<float4 *>(partial + (size_t)blockIdx.x * 2 * c)[i] = t;
    }
}

// out[item] = sum over the slabs of partial[slab][item], item in [0, 2c): 4 items x 64 slab lanes per block; lane g adds slabs
// g, g + 64, ... in that order (four loads in flight), the 64 lane sums are then added by a fixed binary tree through LDS.  This one
// sum is carried in double and rounded once at the end: the fp32 partials are then added exactly, where an fp32 chain over the
// slabs left dbeta two units in the last place off (an ordered serial sum of 33 partials at n = 4099) -- twice what a pairwise
// fp32 sum of the rows has.  dgamma = out[0, c), dbeta = out[c, 2c).
__global__ void __launch_bounds__(kLnFinLanes * kLnFinItems)
ln_bwd_finalize_kernel(const float *__restrict__ partial, int nslab, int c, float *__restrict__ dgamma,
                       float *__restrict__ dbeta) {
    __shared__ double s_sum[kLnFinLanes][kLnFinItems];
    const int il = threadIdx.x & (kLnFinItems - 1), g = threadIdx.x / kLnFinItems;
    const int item = blockIdx.x * kLnFinItems + il;
    double s = 0.0;
    if (item < 2 * c) {
        for (int b0 = g; b0 < nslab; b0 += 4 * kLnFinLanes) {
            float p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int b = b0 + u * kLnFinLanes;
                p[u] = b < nslab ? partial[(size_t)b * 2 * c + item] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s += (double)p[u];
        }
    }
    s_sum[g][il] = s;
    __syncthreads();
    for (int stride = kLnFinLanes / 2; stride >= 1; stride >>= 1) {
        if (g < stride) s_sum[g][il] += s_sum[g + stride][il];
        __syncthreads();
    }
    if (g != 0 || item >= 2 * c) return;
    const float r = (float)s_sum[0][il];
    if (item < c) dgamma[item] = r;
    else dbeta[item - c] = r;
}

static bool ln_supported(int c) { return c >= 32 && c <= 1024 && c % 8 == 0; }

// every row and parameter pointer is moved 16 bytes at a time
static bool ln_aligned(std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

#define U2_LN_SUPPORTED(who)                                                                                       \
    do {                                                                                                           \
        if (!ln_supported(c)) {                                                                                    \
            set_error(who ": c=%d is not supported (a multiple of 8 in 32..1024)", c);                             \
            return 3;                                                                                              \
        }                                                                                                          \
    } while (0)

// the lane-group form of a width: the narrowest group whose lanes cover the row with one 8-channel chunk each
#define U2_LN_DISPATCH(LAUNCH)                 \
    do {                                       \
        const int c8 = c / 8;                  \
        if (c8 <= 8) LAUNCH(8, 1);             \
        else if (c8 <= 16) LAUNCH(16, 1);      \
        else if (c8 <= 32) LAUNCH(32, 1);      \
        else if (c8 <= 64) LAUNCH(64, 1);      \
        else LAUNCH(64, 2);                    \
    } while (0)

template <typename T, bool ADD>
static int ln_forward_impl(const char *who, const T *a, const T *b, const float *w, int64_t n, int32_t c, const float *gamma,
                           const float *beta, float eps, float *mean, float *rstd, T *s_out, T *y, u2mkd_stream_t s) {
    hipStream_t st = as_stream(s);
    const int64_t blocks = ceil_div(n, (int64_t)kLnFwdRows);
    U2_REQUIRE(blocks < ((int64_t)1 << 31), "%s: too many rows (n=%lld)", who, (long long)n);
#define U2_LN_FWD(G, V)                                                                                                   \
    hipLaunchKernelGGL((ln_fwd_kernel<T, G, V, ADD>), dim3((unsigned)blocks), dim3(kLnThreads), 0, st, a, b, w, n, c, gamma, \
                       beta, eps, s_out, y, mean, rstd)
    U2_LN_DISPATCH(U2_LN_FWD);
#undef U2_LN_FWD
    return check_launch(who);
}

template <typename T>
static int ln_backward_impl(const T *dy, const T *x, const T *ds, const float *w, int64_t n, int32_t c, const float *mean,
                            const float *rstd, const float *gamma, float *partial, float *dgamma, float *dbeta, T *dx, T *db,
                            u2mkd_stream_t s) {
    hipStream_t st = as_stream(s);
    const int64_t nslab = u2mkd_ln_num_slabs(n, c);
    U2_REQUIRE(nslab < ((int64_t)1 << 31), "u2mkd_ln_backward: too many rows (n=%lld)", (long long)n);
    const size_t lds = (size_t)(kLnThreads / kWave) * 2 * c * sizeof(float);
#define U2_LN_BWD(G, V)                                                                                                 \
    hipLaunchKernelGGL((ln_bwd_kernel<T, G, V>), dim3((unsigned)nslab), dim3(kLnThreads), lds, st, dy, x, ds, w, n, c, mean, \
                       rstd, gamma, dx, db, partial)
    U2_LN_DISPATCH(U2_LN_BWD);
#undef U2_LN_BWD
    hipLaunchKernelGGL(ln_bwd_finalize_kernel, dim3((unsigned)ceil_div(2 * c, kLnFinItems)), dim3(kLnFinLanes * kLnFinItems), 0,
                       st, partial, (int)nslab, c, dgamma, dbeta);
    return check_launch("u2mkd_ln_backward");
}

}  // namespace u2mkd

using namespace u2mkd;

#define BF(p) reinterpret_cast<const bf16row *>(p)
#define BFW(p) reinterpret_cast<bf16row *>(p)
#define H16(p) reinterpret_cast<const _Float16 *>(p)
#define H16W(p) reinterpret_cast<_Float16 *>(p)
#define F32(p) reinterpret_cast<const float *>(p)
#define F32W(p) reinterpret_cast<float *>(p)
#define U2_ROW_DTYPE(who) U2_REQUIRE(row_dtype >= 0 && row_dtype <= 2, who ": row dtype %d must be 0 (fp32), 1 (bf16) or 2 (fp16)", row_dtype)

extern "C" {

int64_t u2mkd_ln_num_slabs(int64_t n, int32_t c) {
    (void)c;      // (the slab height is the same for every supported width today; callers size the workspace through this entry)
    return n > 0 ? (n + kLnSlabRows - 1) / kLnSlabRows : 0;
}

int u2mkd_ln_forward(const void *x, int32_t row_dtype, int64_t n, int32_t c, const float *gamma, const float *beta, float eps,
                     float *mean, float *rstd, void *y, u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_ln_forward");
    U2_LN_SUPPORTED("u2mkd_ln_forward");
    U2_REQUIRE(n >= 0, "u2mkd_ln_forward: n=%lld", (long long)n);
    if (n == 0) return 0;
    U2_REQUIRE(x && gamma && beta && y, "u2mkd_ln_forward: null pointer");
    U2_REQUIRE((mean == nullptr) == (rstd == nullptr), "u2mkd_ln_forward: mean and rstd go together");
    U2_REQUIRE(ln_aligned({x, gamma, beta, y}), "u2mkd_ln_forward: rows, gamma and beta must be 16-byte aligned");
    if (row_dtype == 2)
        return ln_forward_impl<_Float16, false>("u2mkd_ln_forward", H16(x), nullptr, nullptr, n, c, gamma, beta, eps, mean, rstd,
                                                nullptr, H16W(y), s);
    if (row_dtype == 1)
        return ln_forward_impl<bf16row, false>("u2mkd_ln_forward", BF(x), nullptr, nullptr, n, c, gamma, beta, eps, mean, rstd,
                                               nullptr, BFW(y), s);
    return ln_forward_impl<float, false>("u2mkd_ln_forward", F32(x), nullptr, nullptr, n, c, gamma, beta, eps, mean, rstd,
                                         nullptr, F32W(y), s);
}

int u2mkd_ln_add_forward(const void *a, const void *b, const float *w, int32_t row_dtype, int64_t n, int32_t c,
                         const float *gamma, const float *beta, float eps, float *mean, float *rstd, void *stream_out, void *y,
                         u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_ln_add_forward");
    U2_LN_SUPPORTED("u2mkd_ln_add_forward");
    U2_REQUIRE(n >= 0, "u2mkd_ln_add_forward: n=%lld", (long long)n);
    if (n == 0) return 0;
    U2_REQUIRE(a && b && gamma && beta && stream_out && y, "u2mkd_ln_add_forward: null pointer");
    U2_REQUIRE((mean == nullptr) == (rstd == nullptr), "u2mkd_ln_add_forward: mean and rstd go together");
    U2_REQUIRE(ln_aligned({a, b, gamma, beta, stream_out, y}), "u2mkd_ln_add_forward: rows, gamma and beta must be 16-byte aligned");
    if (row_dtype == 2)
        return ln_forward_impl<_Float16, true>("u2mkd_ln_add_forward", H16(a), H16(b), w, n, c, gamma, beta, eps, mean, rstd,
                                               H16W(stream_out), H16W(y), s);
    if (row_dtype == 1)
        return ln_forward_impl<bf16row, true>("u2mkd_ln_add_forward", BF(a), BF(b), w, n, c, gamma, beta, eps, mean, rstd,
                                              BFW(stream_out), BFW(y), s);
    return ln_forward_impl<float, true>("u2mkd_ln_add_forward", F32(a), F32(b), w, n, c, gamma, beta, eps, mean, rstd,
                                        F32W(stream_out), F32W(y), s);
}

int u2mkd_ln_backward(const void *dy, const void *x, const void *ds, const float *w, int32_t row_dtype, int64_t n, int32_t c,
                      const float *mean, const float *rstd, const float *gamma, float *partial, float *dgamma, float *dbeta,
                      void *dx, void *db, u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_ln_backward");
    U2_LN_SUPPORTED("u2mkd_ln_backward");
    U2_REQUIRE(n >= 0, "u2mkd_ln_backward: n=%lld", (long long)n);
    U2_REQUIRE((w == nullptr) == (db == nullptr), "u2mkd_ln_backward: w and db go together");
    if (n == 0) return 0;
    U2_REQUIRE(dy && x && mean && rstd && gamma && partial && dgamma && dbeta && dx, "u2mkd_ln_backward: null pointer");
    U2_REQUIRE(ln_aligned({dy, x, ds, gamma, partial, dx, db}), "u2mkd_ln_backward: rows, gamma and partial must be 16-byte aligned");
    if (row_dtype == 2)
        return ln_backward_impl<_Float16>(H16(dy), H16(x), H16(ds), w, n, c, mean, rstd, gamma, partial, dgamma, dbeta, H16W(dx),
                                         H16W(db), s);
    if (row_dtype == 1)
        return ln_backward_impl<bf16row>(BF(dy), BF(x), BF(ds), w, n, c, mean, rstd, gamma, partial, dgamma, dbeta, BFW(dx),
                                         BFW(db), s);
    return ln_backward_impl<float>(F32(dy), F32(x), F32(ds), w, n, c, mean, rstd, gamma, partial, dgamma, dbeta, F32W(dx),
                                   F32W(db), s);
}

}  // extern "C"
