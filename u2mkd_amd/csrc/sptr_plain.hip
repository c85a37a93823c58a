// Table-free variable-length window attention, fused: out_i = sum_j softmax_j(q_scale q_i . k_j) v_j over the window of
// token i.  What sptr runs for pe_type 'none' / 'sine' / 'fourier' (sptr/modules.py:53-61): attention_step1, the CSR softmax
// of sptr/utils.py:80-95 and attention_step2, there over M = sum_w L_w^2 pair arrays in HBM; here on the window plan of
// csrc/sptr.hip (tokens sorted by window: sort_idx, wstart, wlen), nothing of size M anywhere.
//
// The same walk as the contextual kernels of csrc/sptr.hip without anything that belongs to the relative-position tables:
// no table image in LDS (the kernels use no LDS at all), no quantised coordinates, no row arithmetic, no histogram strips,
// no matrix-pipe contraction, no slabs and so no workspace.  S lanes per (token, head), S = 1, 2, 4, 8 or 16: lane s walks keys
// s, s + S, ... with its own online-softmax state and the S states are merged by a butterfly (a fixed tree).  The backward
// recomputes the scores from the saved log-sum-exp in two roles: the query role owns dq_i, the key role owns dk_j and dv_j
// (in self-attention the queries of key j are the tokens of its own window), so every gradient row has ONE writer and its
// sum has a fixed order: no atomics, the same bits on every run.
#include "common.h"
#include "sptr_internal.h"

namespace u2mkd {

constexpr int kPlainThreads = 128;

// ---- forward: grid (ceil(n / (128 / S)), h); lse per (sorted position, head) ------------------------------------------------
template <typename T, int S>
__global__ void __launch_bounds__(kPlainThreads)
sptr_plain_fwd_kernel(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v,
                      const int32_t *__restrict__ sort_idx, const int32_t *__restrict__ wstart,
                      const int32_t *__restrict__ wlen, int64_t n, int h, T *__restrict__ out, float *__restrict__ lse,
                      SptrLayout ly) {
    static_assert(S >= 1 && S <= 16 && (S & (S - 1)) == 0, "lanes per token: 1, 2, 4, 8 or 16");
    constexpr int TPB = kPlainThreads / S;
    const int hh = blockIdx.y;
    const int sub = threadIdx.x % S;
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x / S;
    const bool live = p < n;                     // (no early return: the merge shuffles need every lane of the wave)
    const int64_t pp = live ? p : n - 1;
    const int64_t t = sort_idx[pp];
    const size_t hc = ly.ld_qkv;
    float qi[kHd];
    load16(q + t * hc + hh * kHd, qi);
#pragma unroll
    for (int d = 0; d < kHd; ++d) qi[d] *= ly.q_scale;
    const int ws = wstart[pp], wl = live ? wlen[pp] : 0;
    float m = -INFINITY, l = 0.f, acc[kHd];
#pragma unroll
    for (int d = 0; d < kHd; ++d) acc[d] = 0.f;
    // the key's token id one pair ahead (the index load and the row loads behind it are two dependent latencies)
    int64_t tj_n = sub < wl ? sort_idx[ws + sub] : 0;
    for (int jj = sub; jj < wl; jj += S) {
        const int64_t tj = tj_n;
        float kj[kHd], vj[kHd];
        load16(k + tj * hc + hh * kHd, kj);
        load16(v + tj * hc + hh * kHd, vj);
        if (jj + S < wl) tj_n = sort_idx[ws + jj + S];
        float sc = 0.f;
#pragma unroll
        for (int d = 0; d < kHd; ++d) sc += qi[d] * kj[d];
        const float mn = fmaxf(m, sc);
        const float corr = __expf(m - mn), pe = __expf(sc - mn);
        l = l * corr + pe;
#pragma unroll
        for (int d = 0; d < kHd; ++d) acc[d] = acc[d] * corr + pe * vj[d];
        m = mn;
    }
    // merge the S partial softmax states (a lane without keys carries m = -inf, l = 0)
#pragma unroll
    for (int off = S >> 1; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
        const float mn = fmaxf(m, m2);
        const float c1 = m == -INFINITY ? 0.f : __expf(m - mn), c2 = m2 == -INFINITY ? 0.f : __expf(m2 - mn);
        l = l * c1 + l2 * c2;
#pragma unroll
        for (int d = 0; d < kHd; ++d) acc[d] = acc[d] * c1 + __shfl_xor(acc[d], off) * c2;
        m = mn;
    }
    if (live && sub == 0) {
        const float inv = 1.f / l;
#pragma unroll
        for (int d = 0; d < kHd; ++d) acc[d] *= inv;
        store16(out + t * (size_t)ly.ld_out + hh * kHd, acc);
        lse[p * h + hh] = m + __logf(l);
    }
}

// ---- backward: grid (ceil(n / (128 / S)), h, 2); blockIdx.z = 0 the query role (dq), 1 the key role (dk, dv) ----------------
// The two roles are independent (different gradient rows) and share nothing, so one launch covers both.
template <typename T, int S>
__global__ void __launch_bounds__(kPlainThreads)
sptr_plain_bwd_kernel(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v,
                      const T *__restrict__ dout, const float *__restrict__ lse, const float *__restrict__ delta,
                      const int32_t *__restrict__ sort_idx, const int32_t *__restrict__ wstart,
                      const int32_t *__restrict__ wlen, int64_t n, int h, T *__restrict__ dq, T *__restrict__ dk,
                      T *__restrict__ dv, SptrLayout ly) {
    static_assert(S >= 1 && S <= 16 && (S & (S - 1)) == 0, "lanes per token: 1, 2, 4, 8 or 16");
    constexpr int TPB = kPlainThreads / S;
    const int hh = blockIdx.y;
    const int sub = threadIdx.x % S;
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x / S;
    const bool live = p < n;
    const int64_t pp = live ? p : n - 1;
    const int64_t t = sort_idx[pp];
    const size_t hc = ly.ld_qkv, ho = ly.ld_out;
    const int ws = wstart[pp], wl = live ? wlen[pp] : 0;
    if (blockIdx.z == 0) {
        // query role: dq_i = q_scale * sum_j ds_ij k_j,  ds_ij = p_ij (do_i . v_j - delta_i)
        float qi[kHd], doi[kHd], dqi[kHd];
        load16(q + t * hc + hh * kHd, qi);
        load16(dout + t * ho + hh * kHd, doi);
#pragma unroll
        for (int d = 0; d < kHd; ++d) { qi[d] *= ly.q_scale; dqi[d] = 0.f; }
        const float lse_i = lse[pp * h + hh], del_i = delta[pp * h + hh];
        int64_t tj_n = sub < wl ? sort_idx[ws + sub] : 0;          // the pair's index one pair ahead
        for (int jj = sub; jj < wl; jj += S) {
            const int64_t tj = tj_n;
            float kj[kHd], vj[kHd];
            load16(k + tj * hc + hh * kHd, kj);
            load16(v + tj * hc + hh * kHd, vj);
            if (jj + S < wl) tj_n = sort_idx[ws + jj + S];
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < kHd; ++d) { s += qi[d] * kj[d]; dp += doi[d] * vj[d]; }
            const float pr = __expf(s - lse_i);
            const float ds = pr * (dp - del_i);
#pragma unroll
            for (int d = 0; d < kHd; ++d) dqi[d] += ds * kj[d];
        }
#pragma unroll
        for (int off = S >> 1; off >= 1; off >>= 1)
#pragma unroll
            for (int d = 0; d < kHd; ++d) dqi[d] += __shfl_xor(dqi[d], off);
        if (live && sub == 0) {
#pragma unroll
            for (int d = 0; d < kHd; ++d) dqi[d] *= ly.q_scale;      // d(unscaled q) = q_scale * d(q)
            store16(dq + t * (size_t)ly.ld_grad + hh * kHd, dqi);
        }
    } else {
        // key role: dk_j = sum_i ds_ij q_scale q_i,  dv_j = sum_i p_ij do_i over the queries i of the window of j
        float ki[kHd], vi[kHd], dki[kHd], dvi[kHd];
        load16(k + t * hc + hh * kHd, ki);
        load16(v + t * hc + hh * kHd, vi);
#pragma unroll
        for (int d = 0; d < kHd; ++d) { dki[d] = 0.f; dvi[d] = 0.f; }
        int64_t tj_n = 0;                                            // the QUERY of the pair and its two scalars one pair ahead
        float lse_n = 0.f, del_n = 0.f;
        if (sub < wl) {
            const int pj = ws + sub;
            tj_n = sort_idx[pj];
            lse_n = lse[(int64_t)pj * h + hh]; del_n = delta[(int64_t)pj * h + hh];
        }
        for (int jj = sub; jj < wl; jj += S) {
            const int64_t tj = tj_n;
            const float lse_j = lse_n, del_j = del_n;
            float qj[kHd], doj[kHd];
            load16(q + tj * hc + hh * kHd, qj);
            load16(dout + tj * ho + hh * kHd, doj);
            if (jj + S < wl) {
                const int pn = ws + jj + S;
                tj_n = sort_idx[pn];
                lse_n = lse[(int64_t)pn * h + hh]; del_n = delta[(int64_t)pn * h + hh];
            }
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < kHd; ++d) { qj[d] *= ly.q_scale; s += qj[d] * ki[d]; dp += doj[d] * vi[d]; }
            const float pr = __expf(s - lse_j);
            const float ds = pr * (dp - del_j);
#pragma unroll
            for (int d = 0; d < kHd; ++d) { dki[d] += ds * qj[d]; dvi[d] += pr * doj[d]; }
        }
#pragma unroll
        for (int off = S >> 1; off >= 1; off >>= 1)
#pragma unroll
            for (int d = 0; d < kHd; ++d) {
                dki[d] += __shfl_xor(dki[d], off);
                dvi[d] += __shfl_xor(dvi[d], off);
            }
        if (live && sub == 0) {
            store16(dk + t * (size_t)ly.ld_grad + hh * kHd, dki);
            store16(dv + t * (size_t)ly.ld_grad + hh * kHd, dvi);
        }
    }
}

}  // namespace u2mkd

using namespace u2mkd;

// Lanes per (token, head).  The window lengths are known on the device only; the host knows the token count: few tokens
// need the lanes to fill the chip (and are where the windows of hundreds of tokens occur), many tokens fill it anyway.
// U2MKD_SPTR_SPLIT = 1 / 2 / 4 / 8 / 16 overrides (read on every call).
static int plain_split(int64_t n) {
    if (const int forced = sptr_forced_split()) return forced;
    return n < 12000 ? 16 : n < 24000 ? 8 : n < 48000 ? 4 : 2;
}

static int plain_check(const char *who, int64_t n, int h, int hdim, std::initializer_list<int64_t> strides,
                       std::initializer_list<const void *> rows) {
    U2_REQUIRE(hdim == kHd, "%s: head dim %d != 16", who, hdim);
    U2_REQUIRE(h > 0 && h <= 65535, "%s: bad head count %d", who, h);
    U2_REQUIRE(n > 0 && ceil_div(n, kPlainThreads / 16) <= 0x7fffffffLL, "%s: token count %lld out of range", who, (long long)n);
    for (int64_t ld : strides)
        U2_REQUIRE(ld >= (int64_t)h * kHd && ld % 4 == 0, "%s: row stride %lld must be a multiple of 4 floats and hold %d heads",
                   who, (long long)ld, h);
    for (const void *p : rows)                                   // (rows move as 16-byte accesses)
        U2_REQUIRE(reinterpret_cast<uintptr_t>(p) % 16 == 0, "%s: row pointers (q, k, v, out, dout, dq, dk, dv) must be 16-byte aligned", who);
    return 0;
}

extern "C" {

int u2mkd_sptr_plain_forward_strided(const float *q, const float *k, const float *v, int64_t ld_qkv, float q_scale,
                                     const int32_t *sort_idx, const int32_t *wstart, const int32_t *wlen, int64_t n,
                                     int32_t h, int32_t hdim, float *out, int64_t ld_out, float *lse, u2mkd_stream_t s) {
    if (n == 0 || h == 0) return 0;
    U2_REQUIRE(q && k && v && sort_idx && wstart && wlen && out && lse, "u2mkd_sptr_plain_forward: null pointer");
    if (int rc = plain_check("u2mkd_sptr_plain_forward", n, h, hdim, {ld_qkv, ld_out}, {q, k, v, out})) return rc;
    SptrLayout ly{ld_qkv, ld_out, 0, q_scale};
    const int S = plain_split(n);
#define U2_PLAIN_FWD(SS)                                                                                                 \
    hipLaunchKernelGGL((sptr_plain_fwd_kernel<float, SS>), dim3((unsigned)ceil_div(n, kPlainThreads / SS), h),           \
                       dim3(kPlainThreads), 0, as_stream(s), q, k, v, sort_idx, wstart, wlen, n, h, out, lse, ly)
    if (S == 16) U2_PLAIN_FWD(16);
    else if (S == 8) U2_PLAIN_FWD(8);
    else if (S == 4) U2_PLAIN_FWD(4);
    else if (S == 2) U2_PLAIN_FWD(2);
    else U2_PLAIN_FWD(1);
#undef U2_PLAIN_FWD
    return check_launch("u2mkd_sptr_plain_forward");
}

int u2mkd_sptr_plain_backward_strided(const float *q, const float *k, const float *v, int64_t ld_qkv, float q_scale,
                                      const float *out, const float *dout, int64_t ld_out, const float *lse,
                                      const int32_t *sort_idx, const int32_t *wstart, const int32_t *wlen, int64_t n,
                                      int32_t h, int32_t hdim, float *delta, float *dq, float *dk, float *dv,
                                      int64_t ld_grad, u2mkd_stream_t s) {
    if (n == 0 || h == 0) return 0;
    U2_REQUIRE(q && k && v && out && dout && lse && sort_idx && wstart && wlen && delta && dq && dk && dv,
               "u2mkd_sptr_plain_backward: null pointer");
    if (int rc = plain_check("u2mkd_sptr_plain_backward", n, h, hdim, {ld_qkv, ld_out, ld_grad}, {q, k, v, out, dout, dq, dk, dv})) return rc;
    SptrLayout ly{ld_qkv, ld_out, ld_grad, q_scale};
    hipStream_t st = as_stream(s);
    hipLaunchKernelGGL(sptr_delta_kernel<float>, dim3((unsigned)ceil_div(n * h, 256)), dim3(256), 0, st, dout, out, sort_idx,
                       n, h, delta, ld_out);
    const int S = plain_split(n);
#define U2_PLAIN_BWD(SS)                                                                                                 \
    hipLaunchKernelGGL((sptr_plain_bwd_kernel<float, SS>), dim3((unsigned)ceil_div(n, kPlainThreads / SS), h, 2),        \
                       dim3(kPlainThreads), 0, st, q, k, v, dout, lse, delta, sort_idx, wstart, wlen, n, h, dq, dk, dv, ly)
    if (S == 16) U2_PLAIN_BWD(16);
    else if (S == 8) U2_PLAIN_BWD(8);
    else if (S == 4) U2_PLAIN_BWD(4);
    else if (S == 2) U2_PLAIN_BWD(2);
    else U2_PLAIN_BWD(1);
#undef U2_PLAIN_BWD
    return check_launch("u2mkd_sptr_plain_backward");
}

}  // extern "C"
