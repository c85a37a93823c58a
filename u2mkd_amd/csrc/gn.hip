// Reductions over the rows of each SCENE of a [N, C] feature matrix: the rows whose batch index (the last coordinate column)
// is the same.  Serves torchsparse.nn's GroupNorm, GlobalAvgPool and GlobalMaxPool (torchsparse v1.4.0 runs them as a Python
// loop over the batch: a boolean mask, feats[mask], a torch op and a masked write per scene, behind a host read of the batch
// size in every layer and pass).
//
// THE SCENE PLAN (built once per coordinate tensor by the caller): `order` [N] = the rows grouped by scene, ascending row id
// inside a scene (a stable sort by batch index), `seg` [B + 1] the scenes' ranges in it, and a slab table
// (u2mkd_scene_slabs) that cuts every scene into slabs of at most 128 rows of its order; a slab never spans two scenes.
// `order` reads as the identity when the scenes are contiguous.  `bidx` [N] = the batch index of every row.
//
// GroupNorm forward, three launches:
//   slab    one workgroup per slab: per group (mean, M2 around that mean) over the slab's rows x the group's channels
//           (float4 columns x row lanes as in csrc/bn.hip; the slab is re-read for the second moment), kept in double;
//   merge   64 lanes per (scene, group) walk the scene's slabs in slab order and sum, in double, the counts, the means'
//           weighted distances from a pivot (the first slab's mean, which lies among the data) and the second moments
//           around it; a fixed binary tree adds the lanes; mean = K + S / m, M2 = Q - S^2 / m, rstd = bn_invstd;
//   apply   y = (x - mean[b, g]) * rstd[b, g] * gamma_c + beta_c, flat over the rows (b = bidx[row]).
// GroupNorm backward, four launches: slab sums (per channel sum dy and sum dy * xhat; per group sum g and sum g * xhat with
// g = dy * gamma, taken from the channel sums before they are rounded), the ordered merge per (scene, group), the ordered
// sum over all slabs per channel (dgamma, dbeta), and dx = rstd (g - s1 - xhat s2).
// Pooling: slab partials (the column sum in double, or the column max with its row), ordered merge, one division by N_k.
//
// ARITHMETIC as in csrc/bn.hip: every sum over rows or channels is carried in double and rounded once to the fp32 value that is
// stored (the pooled sums stay double until the one division); the elementwise passes carry the arithmetic between a load and
// a store in double and round once.  No atomics, every merge order is fixed: bitwise reproducible.  A float4 column may
// straddle groups (C / G need not be a multiple of 4): every channel looks up its own group.
#include "common.h"

namespace u2mkd {

constexpr int kGnThreads = 256;
constexpr int kGnSlabRows = 128;   // rows per slab (= workgroup of the slab passes)
constexpr int kGnMaxC = 1024;      // c4 <= 256: every float4 column has a thread
constexpr int kGnLanes = 64;       // lanes that walk one scene's slabs in the merge passes

struct GnAcc4 {
    double x, y, z, w;
};
__device__ __forceinline__ GnAcc4 gn_zero() { return GnAcc4{0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ void gn_add(GnAcc4 &a, const GnAcc4 &v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
__device__ __forceinline__ void gn_add(GnAcc4 &a, const float4 &v) {
    a.x += (double)v.x; a.y += (double)v.y; a.z += (double)v.z; a.w += (double)v.w;
}
__device__ __forceinline__ float4 gn_f4(float v) { return make_float4(v, v, v, v); }

// a [B, G] statistic for the four channels of float4 column j (each channel its own group)
__device__ __forceinline__ float4 gn_stat4(const float *__restrict__ stat, int64_t base, int j, int cg, int step = 1) {
    const int ch = 4 * j;
    return make_float4(stat[(base + ch / cg) * step], stat[(base + (ch + 1) / cg) * step], stat[(base + (ch + 2) / cg) * step],
                       stat[(base + (ch + 3) / cg) * step]);
}

// the slab's row ids into LDS; a table entry or a row id outside the matrix is dropped (never addressed)
__device__ __forceinline__ int gn_slab_rows(const int4 sl, const int32_t *__restrict__ order, int64_t n, int *rowid) {
    int rows = sl.z < kGnSlabRows ? sl.z : kGnSlabRows;
    if (sl.x < 0 || sl.y < 0 || (int64_t)sl.y + rows > n) rows = 0;
    for (int i = threadIdx.x; i < rows; i += kGnThreads) {
        const int r = order[sl.y + i];
        rowid[i] = (r >= 0 && (int64_t)r < n) ? r : -1;
    }
    __syncthreads();
    return rows;
}

// the row lanes' sums of every float4 column added in lane order: chs[c] = the slab's sum per channel
__device__ __forceinline__ void gn_cols(GnAcc4 *red, double *chs, const GnAcc4 &s, int c4, int rl, int j, int ry, bool live) {
    if (live) red[ry * c4 + j] = s;
    __syncthreads();
    if (live && ry == 0) {
        GnAcc4 t = gn_zero();
        for (int g = 0; g < rl; ++g) gn_add(t, red[g * c4 + j]);
        chs[4 * j] = t.x; chs[4 * j + 1] = t.y; chs[4 * j + 2] = t.z; chs[4 * j + 3] = t.w;
    }
    __syncthreads();
}

// out[g] = sum over the group's channels of chs[ch] (* scale[ch]): 16 lanes stride the group's channels, lane 0 adds the 16
__device__ __forceinline__ void gn_groups(const double *chs, const float *__restrict__ scale, int groups, int cg, double *out,
                                          double *tmp) {
    const int l = threadIdx.x & 15, gl = threadIdx.x >> 4;
    for (int g0 = 0; g0 < groups; g0 += kGnThreads / 16) {
        const int g = g0 + gl;
        double s = 0.0;
        if (g < groups)
            for (int ch = g * cg + l; ch < (g + 1) * cg; ch += 16) s += scale ? chs[ch] * (double)scale[ch] : chs[ch];
        tmp[threadIdx.x] = s;
        __syncthreads();
        if (g < groups && l == 0) {
            double t = 0.0;
            for (int u = 0; u < 16; ++u) t += tmp[threadIdx.x + u];
            out[g] = t;
        }
        __syncthreads();
    }
}

// ---- the slab table ------------------------------------------------------------------------------------------------------------
// slab_seg [nb + 1]: the scenes' ranges in the slab table; slabs [cap] int4 = (scene, start in order, rows, 0), unused (-1, 0, 0, 0)
__global__ void __launch_bounds__(kGnThreads)
scene_slabs_kernel(const int32_t *__restrict__ seg, int64_t nb, int64_t n, int32_t *slab_seg, int4 *__restrict__ slabs, int64_t cap) {
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int64_t b = 0; b < nb; ++b) {
            slab_seg[b] = (int32_t)acc;
            int64_t cnt = (int64_t)seg[b + 1] - seg[b];
            if (cnt < 0 || seg[b] < 0 || seg[b + 1] > n) cnt = 0;
            const int64_t ns = (cnt + kGnSlabRows - 1) / kGnSlabRows;
            acc = acc + ns <= cap ? acc + ns : acc;      // (cap = ceil(n / 128) + nb holds every scene's slabs)
        }
        slab_seg[nb] = (int32_t)acc;
        __threadfence_block();
    }
    __syncthreads();
    const int64_t used = slab_seg[nb];
    for (int64_t s = threadIdx.x; s < cap; s += kGnThreads) {
        int4 e = make_int4(-1, 0, 0, 0);
        if (s < used) {
            int64_t lo = 0, hi = nb;                     // the scene b with slab_seg[b] <= s < slab_seg[b + 1]
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (slab_seg[mid] <= s) lo = mid; else hi = mid;
            }
            const int64_t start = (int64_t)seg[lo] + (s - slab_seg[lo]) * kGnSlabRows;
            const int64_t rows = min((int64_t)kGnSlabRows, (int64_t)seg[lo + 1] - start);
            if (rows > 0) e = make_int4((int)lo, (int)start, (int)rows, 0);
        }
        slabs[s] = e;
    }
}

// ---- GroupNorm forward ---------------------------------------------------------------------------------------------------------
// partial [nslab][G][2] = (mean, M2 around it) of the slab's rows x the group's channels, kept in DOUBLE: a slab mean rounded to
// fp32 next to a second moment taken around the unrounded one enters the merged variance to FIRST order (2 w (m_b - K) times the
// rounding; 2e-6 of the variance on rows of mean 1e3 and spread 1), and the workspace is a few KB
template <typename T>
__global__ void __launch_bounds__(kGnThreads)
gn_fwd_slab_kernel(const T *__restrict__ x, int64_t n, int c, int groups, const int32_t *__restrict__ order,
                   const int4 *__restrict__ slabs, double *__restrict__ partial) {
    __shared__ GnAcc4 red[kGnThreads];
    __shared__ double chs[kGnMaxC], gmean[kGnMaxC], tmp[kGnThreads];
    __shared__ int rowid[kGnSlabRows];
    double *gm2 = reinterpret_cast<double *>(red);       // (red is free once the columns are summed)
    const int c4 = c >> 2, cg = c / groups, rl = kGnThreads / c4;
    const int j = threadIdx.x % c4, ry = threadIdx.x / c4;
    const bool live = ry < rl;
    const int rows = gn_slab_rows(slabs[blockIdx.x], order, n, rowid);
    double *p = partial + (size_t)blockIdx.x * groups * 2;
    if (rows == 0) {                                     // (the whole workgroup: an unused table entry)
        for (int g = threadIdx.x; g < 2 * groups; g += kGnThreads) p[g] = 0.0;
        return;
    }
    GnAcc4 s = gn_zero();
    if (live)
        for (int rr0 = ry; rr0 < rows; rr0 += 4 * rl) {      // (four rows' loads in flight per trip, summed in row order)
            float4 vv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rr0 + u * rl < rows ? rowid[rr0 + u * rl] : -1;
                vv[u] = r >= 0 ? ld4(x, (int64_t)r * c4 + j) : gn_f4(0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) gn_add(s, vv[u]);
        }
    gn_cols(red, chs, s, c4, rl, j, ry, live);
    gn_groups(chs, nullptr, groups, cg, gmean, tmp);
    for (int g = threadIdx.x; g < groups; g += kGnThreads) gmean[g] /= (double)rows * (double)cg;
    __syncthreads();
    const int ch = 4 * j;
    const double m0 = gmean[ch / cg], m1 = gmean[(ch + 1) / cg], m2 = gmean[(ch + 2) / cg], m3 = gmean[(ch + 3) / cg];
    GnAcc4 q = gn_zero();
    if (live)
        for (int rr0 = ry; rr0 < rows; rr0 += 4 * rl) {
            float4 vv[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rr0 + u * rl < rows ? rowid[rr0 + u * rl] : -1;
                ok[u] = r >= 0;
                vv[u] = ok[u] ? ld4(x, (int64_t)r * c4 + j) : gn_f4(0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
                const double d0 = (double)vv[u].x - m0, d1 = (double)vv[u].y - m1, d2 = (double)vv[u].z - m2, d3 = (double)vv[u].w - m3;
                q.x += d0 * d0; q.y += d1 * d1; q.z += d2 * d2; q.w += d3 * d3;
            }
        }
    gn_cols(red, chs, q, c4, rl, j, ry, live);
    gn_groups(chs, nullptr, groups, cg, gm2, tmp);
    for (int g = threadIdx.x; g < groups; g += kGnThreads) {
        p[2 * g] = gmean[g];
        p[2 * g + 1] = gm2[g];
    }
}

// one (scene, group) per 64 lanes; mean, rstd [nb][G] (a scene without rows: 0, 0 -- nothing reads them)
__global__ void __launch_bounds__(kGnThreads)
gn_fwd_merge_kernel(const double *__restrict__ partial, const int4 *__restrict__ slabs, const int32_t *__restrict__ slab_seg,
                    const int32_t *__restrict__ seg, int64_t nb, int groups, int cg, float eps, float *__restrict__ mean,
                    float *__restrict__ rstd) {
    __shared__ double s_s[kGnThreads / kGnLanes][kGnLanes], s_q[kGnThreads / kGnLanes][kGnLanes];
    const int pl = threadIdx.x / kGnLanes, l = threadIdx.x % kGnLanes;
    const int64_t pair = (int64_t)blockIdx.x * (kGnThreads / kGnLanes) + pl;
    const bool valid = pair < nb * groups;
    const int64_t b = valid ? pair / groups : 0;
    const int g = valid ? (int)(pair % groups) : 0;
    const int s0 = valid ? slab_seg[b] : 0, s1 = valid ? slab_seg[b + 1] : 0;
    const double pivot = s1 > s0 ? partial[((size_t)s0 * groups + g) * 2] : 0.0;
    double ss = 0.0, qq = 0.0;
    for (int si = s0 + l; si < s1; si += kGnLanes) {
        const double w = (double)slabs[si].z * (double)cg;
        const double d = partial[((size_t)si * groups + g) * 2] - pivot;
        ss += w * d;
        qq += partial[((size_t)si * groups + g) * 2 + 1] + w * d * d;
    }
    s_s[pl][l] = ss; s_q[pl][l] = qq;
    __syncthreads();
    for (int stride = kGnLanes / 2; stride >= 1; stride >>= 1) {      // (fixed binary tree over the 64 lanes)
        if (l < stride) {
            s_s[pl][l] += s_s[pl][l + stride];
            s_q[pl][l] += s_q[pl][l + stride];
        }
        __syncthreads();
    }
    if (l != 0 || !valid) return;
    const double m = ((double)seg[b + 1] - (double)seg[b]) * (double)cg;
    if (!(m > 0.0) || s1 <= s0) {
        mean[pair] = 0.f; rstd[pair] = 0.f;
        return;
    }
    const double shift = s_s[pl][0] / m;
    const double m2 = s_q[pl][0] - s_s[pl][0] * shift;
    mean[pair] = (float)(pivot + shift);
    rstd[pair] = bn_invstd((m2 > 0.0 ? m2 : 0.0) / m + (double)eps);
}

__device__ __forceinline__ float gn_out(float v, float m, float r, float g, float b) {
    return (float)(((double)v - (double)m) * (double)r * (double)g + (double)b);
}

// a row whose batch index is outside [0, nb) belongs to no scene: zeros, as the loop formulation leaves it
template <typename T>
__global__ void gn_apply_kernel(const T *__restrict__ x, int64_t total4, int c4, int groups, int cg,
                                const int32_t *__restrict__ bidx, int64_t nb, const float *__restrict__ mean,
                                const float *__restrict__ rstd, const float *__restrict__ gamma, const float *__restrict__ beta,
                                T *__restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    const int j = (int)(t % c4);
    const int b = bidx[t / c4];
    if (b < 0 || b >= nb) {
        st4(y, t, gn_f4(0.f));
        return;
    }
    const float4 v = ld4(x, t);
    const float4 m = gn_stat4(mean, (int64_t)b * groups, j, cg), r = gn_stat4(rstd, (int64_t)b * groups, j, cg);
    const float4 g = gamma ? *reinterpret_cast<const float4 *>(gamma + 4 * j) : gn_f4(1.f);
    const float4 bt = beta ? *reinterpret_cast<const float4 *>(beta + 4 * j) : gn_f4(0.f);
    st4(y, t, make_float4(gn_out(v.x, m.x, r.x, g.x, bt.x), gn_out(v.y, m.y, r.y, g.y, bt.y), gn_out(v.z, m.z, r.z, g.z, bt.z),
                          gn_out(v.w, m.w, r.w, g.w, bt.w)));
}

// ---- GroupNorm backward --------------------------------------------------------------------------------------------------------
// pc [nslab][2][C] = (sum dy, sum dy * xhat) per channel; pg [nslab][G][2] = (sum g, sum g * xhat) per group, g = dy * gamma
template <typename T>
__global__ void __launch_bounds__(kGnThreads)
gn_bwd_slab_kernel(const T *__restrict__ dy, const T *__restrict__ x, int64_t n, int c, int groups,
                   const int32_t *__restrict__ order, const int4 *__restrict__ slabs, const float *__restrict__ mean,
                   const float *__restrict__ rstd, const float *__restrict__ gamma, float *__restrict__ pc,
                   float *__restrict__ pg) {
    __shared__ GnAcc4 red1[kGnThreads], red2[kGnThreads];
    __shared__ double chs1[kGnMaxC], chs2[kGnMaxC], tmp[kGnThreads];
    __shared__ int rowid[kGnSlabRows];
    double *go1 = reinterpret_cast<double *>(red1), *go2 = reinterpret_cast<double *>(red2);
    const int c4 = c >> 2, cg = c / groups, rl = kGnThreads / c4;
    const int j = threadIdx.x % c4, ry = threadIdx.x / c4;
    const bool live = ry < rl;
    const int4 sl = slabs[blockIdx.x];
    const int rows = gn_slab_rows(sl, order, n, rowid);
    float *p_c = pc + (size_t)blockIdx.x * 2 * c, *p_g = pg + (size_t)blockIdx.x * groups * 2;
    if (rows == 0) {
        for (int i = threadIdx.x; i < 2 * c; i += kGnThreads) p_c[i] = 0.f;
        for (int i = threadIdx.x; i < 2 * groups; i += kGnThreads) p_g[i] = 0.f;
        return;
    }
    GnAcc4 s1 = gn_zero(), s2 = gn_zero();
    if (live) {
        const float4 m = gn_stat4(mean, (int64_t)sl.x * groups, j, cg), r = gn_stat4(rstd, (int64_t)sl.x * groups, j, cg);
        for (int rr0 = ry; rr0 < rows; rr0 += 4 * rl) {
            float4 vv[4], dd[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rw = rr0 + u * rl < rows ? rowid[rr0 + u * rl] : -1;
                vv[u] = rw >= 0 ? ld4(x, (int64_t)rw * c4 + j) : gn_f4(0.f);
                dd[u] = rw >= 0 ? ld4(dy, (int64_t)rw * c4 + j) : gn_f4(0.f);       // (a dropped row adds exact zeros)
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 v = vv[u], d = dd[u];
                gn_add(s1, d);
                s2.x += (double)d.x * (((double)v.x - (double)m.x) * (double)r.x);
                s2.y += (double)d.y * (((double)v.y - (double)m.y) * (double)r.y);
                s2.z += (double)d.z * (((double)v.z - (double)m.z) * (double)r.z);
                s2.w += (double)d.w * (((double)v.w - (double)m.w) * (double)r.w);
            }
        }
    }
    gn_cols(red1, chs1, s1, c4, rl, j, ry, live);
    gn_cols(red2, chs2, s2, c4, rl, j, ry, live);
    for (int i = threadIdx.x; i < c; i += kGnThreads) {
        p_c[i] = (float)chs1[i];
        p_c[c + i] = (float)chs2[i];
    }
    gn_groups(chs1, gamma, groups, cg, go1, tmp);
    gn_groups(chs2, gamma, groups, cg, go2, tmp);
    for (int g = threadIdx.x; g < groups; g += kGnThreads) {
        p_g[2 * g] = (float)go1[g];
        p_g[2 * g + 1] = (float)go2[g];
    }
}

// sums [nb][G][2] = (s1, s2) = (sum g, sum g * xhat) / m of the scene, m = (C / G) N_k; a scene without rows: 0, 0
__global__ void __launch_bounds__(kGnThreads)
gn_bwd_merge_groups_kernel(const float *__restrict__ pg, const int32_t *__restrict__ slab_seg, const int32_t *__restrict__ seg,
                           int64_t nb, int groups, int cg, float *__restrict__ sums) {
    __shared__ double s_1[kGnThreads / kGnLanes][kGnLanes], s_2[kGnThreads / kGnLanes][kGnLanes];
    const int pl = threadIdx.x / kGnLanes, l = threadIdx.x % kGnLanes;
    const int64_t pair = (int64_t)blockIdx.x * (kGnThreads / kGnLanes) + pl;
    const bool valid = pair < nb * groups;
    const int64_t b = valid ? pair / groups : 0;
    const int g = valid ? (int)(pair % groups) : 0;
    const int s0 = valid ? slab_seg[b] : 0, s1 = valid ? slab_seg[b + 1] : 0;
    double a1 = 0.0, a2 = 0.0;
    for (int si = s0 + l; si < s1; si += kGnLanes) {
        a1 += (double)pg[((size_t)si * groups + g) * 2];
        a2 += (double)pg[((size_t)si * groups + g) * 2 + 1];
    }
    s_1[pl][l] = a1; s_2[pl][l] = a2;
    __syncthreads();
    for (int stride = kGnLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride) {
            s_1[pl][l] += s_1[pl][l + stride];
            s_2[pl][l] += s_2[pl][l + stride];
        }
        __syncthreads();
    }
    if (l != 0 || !valid) return;
    const double m = ((double)seg[b + 1] - (double)seg[b]) * (double)cg;
    sums[2 * pair] = m > 0.0 ? (float)(s_1[pl][0] / m) : 0.f;
    sums[2 * pair + 1] = m > 0.0 ? (float)(s_2[pl][0] / m) : 0.f;
}

// dbeta [C], dgamma [C]: the channel sums of every slab, 64 lanes per channel in slab order, fixed tree
__global__ void __launch_bounds__(kGnThreads)
gn_bwd_merge_channels_kernel(const float *__restrict__ pc, int64_t nslab, int c, float *__restrict__ dgamma,
                             float *__restrict__ dbeta) {
    __shared__ double s_1[kGnLanes][4], s_2[kGnLanes][4];
    const int cl = threadIdx.x & 3, l = threadIdx.x >> 2;
    const int ch = blockIdx.x * 4 + cl;
    double a1 = 0.0, a2 = 0.0;
    if (ch < c)
        for (int64_t si = l; si < nslab; si += kGnLanes) {
            a1 += (double)pc[(size_t)si * 2 * c + ch];
            a2 += (double)pc[(size_t)si * 2 * c + c + ch];
        }
    s_1[l][cl] = a1; s_2[l][cl] = a2;
    __syncthreads();
    for (int stride = kGnLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride) {
            s_1[l][cl] += s_1[l + stride][cl];
            s_2[l][cl] += s_2[l + stride][cl];
        }
        __syncthreads();
    }
    if (l != 0 || ch >= c) return;
    dbeta[ch] = (float)s_1[0][cl];
    dgamma[ch] = (float)s_2[0][cl];
}

__device__ __forceinline__ float gn_dx(float v, float d, float m, float r, float g, float s1, float s2) {
    const double xh = ((double)v - (double)m) * (double)r;
    return (float)((double)r * ((double)d * (double)g - (double)s1 - xh * (double)s2));
}

template <typename T>
__global__ void gn_bwd_apply_kernel(const T *__restrict__ dy, const T *__restrict__ x, int64_t total4, int c4, int groups, int cg,
                                    const int32_t *__restrict__ bidx, int64_t nb, const float *__restrict__ mean,
                                    const float *__restrict__ rstd, const float *__restrict__ gamma,
                                    const float *__restrict__ sums, T *__restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    const int j = (int)(t % c4);
    const int b = bidx[t / c4];
    if (b < 0 || b >= nb) {
        st4(dx, t, gn_f4(0.f));
        return;
    }
    const float4 v = ld4(x, t), d = ld4(dy, t);
    const int64_t base = (int64_t)b * groups;
    const float4 m = gn_stat4(mean, base, j, cg), r = gn_stat4(rstd, base, j, cg);
    const float4 a1 = gn_stat4(sums, base, j, cg, 2), a2 = gn_stat4(sums + 1, base, j, cg, 2);
    const float4 g = gamma ? *reinterpret_cast<const float4 *>(gamma + 4 * j) : gn_f4(1.f);
    st4(dx, t, make_float4(gn_dx(v.x, d.x, m.x, r.x, g.x, a1.x, a2.x), gn_dx(v.y, d.y, m.y, r.y, g.y, a1.y, a2.y),
                           gn_dx(v.z, d.z, m.z, r.z, g.z, a1.z, a2.z), gn_dx(v.w, d.w, m.w, r.w, g.w, a1.w, a2.w)));
}

// ---- pooling -------------------------------------------------------------------------------------------------------------------
// whether (a, row ra) takes the place of (b, row rb) as a column's maximum: a NaN beats every number, equal values and two NaNs
// keep the smaller row (torch.max: NaN propagates; the gradient goes to the first of the maxima); row -1 = nothing yet
__device__ __forceinline__ bool gn_better(float a, int ra, float b, int rb) {
    if (ra < 0) return false;
    if (rb < 0) return true;
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ra < rb);
    return a > b || (a == b && ra < rb);
}
__device__ __forceinline__ void gn_take(float &b, int &rb, float a, int ra) {
    if (gn_better(a, ra, b, rb)) { b = a; rb = ra; }
}

// avg: psum [nslab][C] double = the slab's column sums
template <typename T>
__global__ void __launch_bounds__(kGnThreads)
pool_sum_slab_kernel(const T *__restrict__ x, int64_t n, int c, const int32_t *__restrict__ order,
                     const int4 *__restrict__ slabs, double *__restrict__ psum) {
    __shared__ GnAcc4 red[kGnThreads];
    __shared__ double chs[kGnMaxC];
    __shared__ int rowid[kGnSlabRows];
    const int c4 = c >> 2, rl = kGnThreads / c4;
    const int j = threadIdx.x % c4, ry = threadIdx.x / c4;
    const bool live = ry < rl;
    const int rows = gn_slab_rows(slabs[blockIdx.x], order, n, rowid);
    double *p = psum + (size_t)blockIdx.x * c;
    if (rows == 0) {
        for (int i = threadIdx.x; i < c; i += kGnThreads) p[i] = 0.0;
        return;
    }
    GnAcc4 s = gn_zero();
    if (live)
        for (int rr0 = ry; rr0 < rows; rr0 += 4 * rl) {
            float4 vv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rr0 + u * rl < rows ? rowid[rr0 + u * rl] : -1;
                vv[u] = r >= 0 ? ld4(x, (int64_t)r * c4 + j) : gn_f4(0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) gn_add(s, vv[u]);
        }
    gn_cols(red, chs, s, c4, rl, j, ry, live);
    for (int i = threadIdx.x; i < c; i += kGnThreads) p[i] = chs[i];
}

// max: pmax [nslab][C] = the slab's column maxima, parg [nslab][C] = their rows (-1: no row)
template <typename T>
__global__ void __launch_bounds__(kGnThreads)
pool_max_slab_kernel(const T *__restrict__ x, int64_t n, int c, const int32_t *__restrict__ order,
                     const int4 *__restrict__ slabs, float *__restrict__ pmax, int32_t *__restrict__ parg) {
    __shared__ float4 redv[kGnThreads];
    __shared__ int4 redr[kGnThreads];
    __shared__ int rowid[kGnSlabRows];
    const int c4 = c >> 2, rl = kGnThreads / c4;
    const int j = threadIdx.x % c4, ry = threadIdx.x / c4;
    const bool live = ry < rl;
    const int rows = gn_slab_rows(slabs[blockIdx.x], order, n, rowid);
    float *pv = pmax + (size_t)blockIdx.x * c;
    int32_t *pr = parg + (size_t)blockIdx.x * c;
    if (rows == 0) {
        for (int i = threadIdx.x; i < c; i += kGnThreads) { pv[i] = -INFINITY; pr[i] = -1; }
        return;
    }
    float4 bv = gn_f4(-INFINITY);
    int4 br = make_int4(-1, -1, -1, -1);
    if (live)
        for (int rr = ry; rr < rows; rr += rl) {
            const int r = rowid[rr];
            if (r < 0) continue;
            const float4 v = ld4(x, (int64_t)r * c4 + j);
            gn_take(bv.x, br.x, v.x, r); gn_take(bv.y, br.y, v.y, r); gn_take(bv.z, br.z, v.z, r); gn_take(bv.w, br.w, v.w, r);
        }
    if (live) { redv[ry * c4 + j] = bv; redr[ry * c4 + j] = br; }
    __syncthreads();
    if (live && ry == 0) {
        for (int g = 1; g < rl; ++g) {
            const float4 v = redv[g * c4 + j];
            const int4 r = redr[g * c4 + j];
            gn_take(bv.x, br.x, v.x, r.x); gn_take(bv.y, br.y, v.y, r.y); gn_take(bv.z, br.z, v.z, r.z); gn_take(bv.w, br.w, v.w, r.w);
        }
        *reinterpret_cast<float4 *>(pv + 4 * j) = bv;
        *reinterpret_cast<int4 *>(pr + 4 * j) = br;
    }
}

// out [nb][C]: grid (ceil(C / 4), nb), 64 lanes per (scene, channel) over the scene's slabs in slab order, fixed tree
__global__ void __launch_bounds__(kGnThreads)
pool_sum_merge_kernel(const double *__restrict__ psum, const int32_t *__restrict__ slab_seg, const int32_t *__restrict__ seg, int c,
                      float *__restrict__ out) {
    __shared__ double s_1[kGnLanes][4];
    const int cl = threadIdx.x & 3, l = threadIdx.x >> 2;
    const int ch = blockIdx.x * 4 + cl, b = blockIdx.y;
    const int s0 = slab_seg[b], s1 = slab_seg[b + 1];
    double a = 0.0;
    if (ch < c)
        for (int si = s0 + l; si < s1; si += kGnLanes) a += psum[(size_t)si * c + ch];
    s_1[l][cl] = a;
    __syncthreads();
    for (int stride = kGnLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride) s_1[l][cl] += s_1[l + stride][cl];
        __syncthreads();
    }
    if (l != 0 || ch >= c) return;
    // the one division: a scene without rows gives 0 / 0 = NaN, as torch.mean of nothing does
    out[(size_t)b * c + ch] = (float)(s_1[0][cl] / ((double)seg[b + 1] - (double)seg[b]));
}

__global__ void __launch_bounds__(kGnThreads)
pool_max_merge_kernel(const float *__restrict__ pmax, const int32_t *__restrict__ parg, const int32_t *__restrict__ slab_seg, int c,
                      float *__restrict__ out, int32_t *__restrict__ arg) {
    __shared__ float s_v[kGnLanes][4];
    __shared__ int s_r[kGnLanes][4];
    const int cl = threadIdx.x & 3, l = threadIdx.x >> 2;
    const int ch = blockIdx.x * 4 + cl, b = blockIdx.y;
    const int s0 = slab_seg[b], s1 = slab_seg[b + 1];
    float bv = -INFINITY;       // (the identity: a scene without rows)
    int br = -1;
    if (ch < c)
        for (int si = s0 + l; si < s1; si += kGnLanes) gn_take(bv, br, pmax[(size_t)si * c + ch], parg[(size_t)si * c + ch]);
    s_v[l][cl] = bv; s_r[l][cl] = br;
    __syncthreads();
    for (int stride = kGnLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride) {
            float v = s_v[l][cl];
            int r = s_r[l][cl];
            gn_take(v, r, s_v[l + stride][cl], s_r[l + stride][cl]);
            s_v[l][cl] = v; s_r[l][cl] = r;
        }
        __syncthreads();
    }
    if (l != 0 || ch >= c) return;
    out[(size_t)b * c + ch] = s_v[0][cl];
    arg[(size_t)b * c + ch] = s_r[0][cl];
}

// dx[row] = dy[b] / N_b (one division in double, one rounding); a row of no scene: zeros
template <typename T>
__global__ void pool_avg_bwd_kernel(const float *__restrict__ dy, int64_t total4, int c4, const int32_t *__restrict__ bidx,
                                    const int32_t *__restrict__ seg, int64_t nb, T *__restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    const int j = (int)(t % c4);
    const int b = bidx[t / c4];
    if (b < 0 || b >= nb) {
        st4(dx, t, gn_f4(0.f));
        return;
    }
    const double cnt = (double)seg[b + 1] - (double)seg[b];
    const float4 d = *reinterpret_cast<const float4 *>(dy + ((size_t)b * c4 + j) * 4);
    st4(dx, t, make_float4((float)((double)d.x / cnt), (float)((double)d.y / cnt), (float)((double)d.z / cnt), (float)((double)d.w / cnt)));
}

template <typename T> __device__ __forceinline__ void gn_st1(T *p, int64_t i, float v);
template <> __device__ __forceinline__ void gn_st1<float>(float *p, int64_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void gn_st1<bf16row>(bf16row *p, int64_t i, float v) {
    const __bf16 h = (__bf16)v;
    p[i].v = __builtin_bit_cast(unsigned short, h);
}
template <> __device__ __forceinline__ void gn_st1<_Float16>(_Float16 *p, int64_t i, float v) { p[i] = (_Float16)v; }

// dx (zero-filled by the caller's stream before this launch) takes dy[b, ch] at the saved row of the maximum
template <typename T>
__global__ void pool_max_bwd_kernel(const float *__restrict__ dy, const int32_t *__restrict__ arg, int64_t total, int c, int64_t n,
                                    T *__restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int r = arg[t];
    if (r < 0 || (int64_t)r >= n) return;
    gn_st1(dx, (int64_t)r * c + (t % c), dy[t]);
}

// ---- launch sequences ----------------------------------------------------------------------------------------------------------
static bool gn_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
static int gn_forward_impl(const T *x, int64_t n, int32_t c, int32_t groups, const int32_t *bidx, const int32_t *order,
                           const int32_t *seg, const int32_t *slab_seg, const int32_t *slabs, int64_t nslab, int64_t nb,
                           const float *gamma, const float *beta, float eps, double *partial, float *mean, float *rstd, T *y,
                           u2mkd_stream_t s) {
    hipStream_t st = as_stream(s);
    const int4 *tab = reinterpret_cast<const int4 *>(slabs);
    hipLaunchKernelGGL(gn_fwd_slab_kernel<T>, dim3((unsigned)nslab), dim3(kGnThreads), 0, st, x, n, c, groups, order, tab, partial);
    hipLaunchKernelGGL(gn_fwd_merge_kernel, dim3((unsigned)ceil_div(nb * groups, kGnThreads / kGnLanes)), dim3(kGnThreads), 0, st,
                       partial, tab, slab_seg, seg, nb, groups, c / groups, eps, mean, rstd);
    const int64_t total4 = n * (c / 4);
    hipLaunchKernelGGL(gn_apply_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, x, total4, c / 4, groups,
                       c / groups, bidx, nb, mean, rstd, gamma, beta, y);
    return check_launch("u2mkd_gn_forward");
}

template <typename T>
static int gn_backward_impl(const T *dy, const T *x, int64_t n, int32_t c, int32_t groups, const int32_t *bidx,
                            const int32_t *order, const int32_t *seg, const int32_t *slab_seg, const int32_t *slabs, int64_t nslab,
                            int64_t nb, const float *mean, const float *rstd, const float *gamma, float *partial, float *sums,
                            float *dgamma, float *dbeta, T *dx, u2mkd_stream_t s) {
    hipStream_t st = as_stream(s);
    const int4 *tab = reinterpret_cast<const int4 *>(slabs);
    float *pc = partial, *pg = partial + (size_t)nslab * 2 * c;
    hipLaunchKernelGGL(gn_bwd_slab_kernel<T>, dim3((unsigned)nslab), dim3(kGnThreads), 0, st, dy, x, n, c, groups, order, tab, mean,
                       rstd, gamma, pc, pg);
    hipLaunchKernelGGL(gn_bwd_merge_groups_kernel, dim3((unsigned)ceil_div(nb * groups, kGnThreads / kGnLanes)), dim3(kGnThreads), 0,
                       st, pg, slab_seg, seg, nb, groups, c / groups, sums);
    if (dgamma)
        hipLaunchKernelGGL(gn_bwd_merge_channels_kernel, dim3((unsigned)ceil_div(c, 4)), dim3(kGnThreads), 0, st, pc, nslab, c, dgamma,
                           dbeta);
    const int64_t total4 = n * (c / 4);
    hipLaunchKernelGGL(gn_bwd_apply_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, dy, x, total4, c / 4, groups,
                       c / groups, bidx, nb, mean, rstd, gamma, sums, dx);
    return check_launch("u2mkd_gn_backward");
}

template <typename T>
static int pool_forward_impl(const T *x, int64_t n, int32_t c, int32_t mode, const int32_t *order, const int32_t *seg,
                             const int32_t *slab_seg, const int32_t *slabs, int64_t nslab, int64_t nb, void *partial, float *out,
                             int32_t *arg, u2mkd_stream_t s) {
    hipStream_t st = as_stream(s);
    const int4 *tab = reinterpret_cast<const int4 *>(slabs);
    const dim3 mgrid((unsigned)ceil_div(c, 4), (unsigned)nb);
    if (mode == 0) {
        double *psum = reinterpret_cast<double *>(partial);
        hipLaunchKernelGGL(pool_sum_slab_kernel<T>, dim3((unsigned)nslab), dim3(kGnThreads), 0, st, x, n, c, order, tab, psum);
        hipLaunchKernelGGL(pool_sum_merge_kernel, mgrid, dim3(kGnThreads), 0, st, psum, slab_seg, seg, c, out);
    } else {
        float *pmax = reinterpret_cast<float *>(partial);
        int32_t *parg = reinterpret_cast<int32_t *>(pmax + (size_t)nslab * c);
        hipLaunchKernelGGL(pool_max_slab_kernel<T>, dim3((unsigned)nslab), dim3(kGnThreads), 0, st, x, n, c, order, tab, pmax, parg);
        hipLaunchKernelGGL(pool_max_merge_kernel, mgrid, dim3(kGnThreads), 0, st, pmax, parg, slab_seg, c, out, arg);
    }
    return check_launch("u2mkd_scene_pool_forward");
}

template <typename T>
static int pool_backward_impl(const float *dy, int64_t n, int32_t c, int32_t mode, const int32_t *bidx, const int32_t *seg,
                              const int32_t *arg, int64_t nb, T *dx, u2mkd_stream_t s) {
    hipStream_t st = as_stream(s);
    if (mode == 0) {
        const int64_t total4 = n * (c / 4);
        hipLaunchKernelGGL(pool_avg_bwd_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, dy, total4, c / 4, bidx,
                           seg, nb, dx);
    } else {
        (void)hipMemsetAsync(dx, 0, (size_t)n * c * sizeof(T), st);
        const int64_t total = nb * c;
        if (total > 0)
            hipLaunchKernelGGL(pool_max_bwd_kernel<T>, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, dy, arg, total, c, n, dx);
    }
    return check_launch("u2mkd_scene_pool_backward");
}

}  // namespace u2mkd

using namespace u2mkd;

#define GN_ROWS(who)                                                                                                              \
    U2_REQUIRE(row_dtype >= 0 && row_dtype <= 2, who ": row dtype %d must be 0 (fp32), 1 (bf16) or 2 (fp16)", row_dtype);          \
    U2_REQUIRE(c > 0 && c % 4 == 0 && c <= kGnMaxC, who ": c=%d must be a multiple of 4 in 4..1024", c);                          \
    U2_REQUIRE(n >= 0 && n * (int64_t)c < ((int64_t)1 << 40) && n < ((int64_t)1 << 31), who ": n=%lld rows", (long long)n);        \
    U2_REQUIRE(nb >= 0 && nb < 65536, who ": %lld scenes (at most 65535)", (long long)nb)
// dispatch over the rows' dtype: CALL(T) with T = float, bf16row or _Float16
#define GN_BY_DTYPE(CALL)                                                                                                         \
    (row_dtype == 2 ? CALL(_Float16) : row_dtype == 1 ? CALL(bf16row) : CALL(float))

extern "C" {

int64_t u2mkd_scene_num_slabs(int64_t n, int64_t nb) {
    return n > 0 && nb > 0 ? (n + kGnSlabRows - 1) / kGnSlabRows + nb : 0;
}

int u2mkd_scene_slabs(const int32_t *seg, int64_t nb, int64_t n, int32_t *slab_seg, int32_t *slabs, int64_t nslab,
                      u2mkd_stream_t s) {
    U2_REQUIRE(nb >= 0 && nb < 65536 && n >= 0 && n < ((int64_t)1 << 31), "u2mkd_scene_slabs: %lld scenes, %lld rows",
               (long long)nb, (long long)n);
    U2_REQUIRE(nslab == u2mkd_scene_num_slabs(n, nb), "u2mkd_scene_slabs: the table holds %lld slabs, u2mkd_scene_num_slabs gives %lld",
               (long long)nslab, (long long)u2mkd_scene_num_slabs(n, nb));
    if (nslab == 0) return 0;
    U2_REQUIRE(seg && slab_seg && slabs, "u2mkd_scene_slabs: null pointer");
    U2_REQUIRE(gn_aligned16(slabs), "u2mkd_scene_slabs: the slab table must be 16-byte aligned");
    hipLaunchKernelGGL(scene_slabs_kernel, dim3(1), dim3(kGnThreads), 0, as_stream(s), seg, nb, n, slab_seg,
                       reinterpret_cast<int4 *>(slabs), nslab);
    return check_launch("u2mkd_scene_slabs");
}

int u2mkd_gn_forward(const void *x, int32_t row_dtype, int64_t n, int32_t c, int32_t groups, const int32_t *bidx,
                     const int32_t *order, const int32_t *seg, const int32_t *slab_seg, const int32_t *slabs, int64_t nslab,
                     int64_t nb, const float *gamma, const float *beta, float eps, void *partial, float *mean, float *rstd,
                     void *y, u2mkd_stream_t s) {
    GN_ROWS("u2mkd_gn_forward");
    U2_REQUIRE(groups > 0 && c % groups == 0, "u2mkd_gn_forward: %d groups do not divide c=%d", groups, c);
    U2_REQUIRE(nslab == u2mkd_scene_num_slabs(n, nb), "u2mkd_gn_forward: nslab=%lld is not u2mkd_scene_num_slabs(n, nb)", (long long)nslab);
    if (n == 0 || nb == 0) return 0;
    U2_REQUIRE(x && bidx && order && seg && slab_seg && slabs && partial && mean && rstd && y, "u2mkd_gn_forward: null pointer");
    U2_REQUIRE(gn_aligned16(x) && gn_aligned16(y) && gn_aligned16(slabs) && gn_aligned16(gamma) && gn_aligned16(beta) && gn_aligned16(partial),
               "u2mkd_gn_forward: rows, parameters, the slab table and the workspace must be 16-byte aligned");
#define GN_CALL(T)                                                                                                                \
    gn_forward_impl<T>(reinterpret_cast<const T *>(x), n, c, groups, bidx, order, seg, slab_seg, slabs, nslab, nb, gamma, beta, eps, \
                       reinterpret_cast<double *>(partial), mean, rstd, reinterpret_cast<T *>(y), s)
    return GN_BY_DTYPE(GN_CALL);
#undef GN_CALL
}

int u2mkd_gn_backward(const void *dy, const void *x, int32_t row_dtype, int64_t n, int32_t c, int32_t groups, const int32_t *bidx,
                      const int32_t *order, const int32_t *seg, const int32_t *slab_seg, const int32_t *slabs, int64_t nslab,
                      int64_t nb, const float *mean, const float *rstd, const float *gamma, float *partial, float *sums,
                      float *dgamma, float *dbeta, void *dx, u2mkd_stream_t s) {
    GN_ROWS("u2mkd_gn_backward");
    U2_REQUIRE(groups > 0 && c % groups == 0, "u2mkd_gn_backward: %d groups do not divide c=%d", groups, c);
    U2_REQUIRE(nslab == u2mkd_scene_num_slabs(n, nb), "u2mkd_gn_backward: nslab=%lld is not u2mkd_scene_num_slabs(n, nb)", (long long)nslab);
    U2_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "u2mkd_gn_backward: dgamma and dbeta go together");
    if (n == 0 || nb == 0) return 0;
    U2_REQUIRE(dy && x && bidx && order && seg && slab_seg && slabs && mean && rstd && partial && sums && dx,
               "u2mkd_gn_backward: null pointer");
    U2_REQUIRE(gn_aligned16(dy) && gn_aligned16(x) && gn_aligned16(dx) && gn_aligned16(slabs) && gn_aligned16(gamma),
               "u2mkd_gn_backward: rows, gamma and the slab table must be 16-byte aligned");
#define GN_CALL(T)                                                                                                                \
    gn_backward_impl<T>(reinterpret_cast<const T *>(dy), reinterpret_cast<const T *>(x), n, c, groups, bidx, order, seg, slab_seg,    \
                        slabs, nslab, nb, mean, rstd, gamma, partial, sums, dgamma, dbeta, reinterpret_cast<T *>(dx), s)
    return GN_BY_DTYPE(GN_CALL);
#undef GN_CALL
}

int u2mkd_scene_pool_forward(const void *x, int32_t row_dtype, int64_t n, int32_t c, int32_t mode, const int32_t *order,
                             const int32_t *seg, const int32_t *slab_seg, const int32_t *slabs, int64_t nslab, int64_t nb,
                             void *partial, float *out, int32_t *arg, u2mkd_stream_t s) {
    GN_ROWS("u2mkd_scene_pool_forward");
    U2_REQUIRE(mode == 0 || mode == 1, "u2mkd_scene_pool_forward: mode %d must be 0 (mean) or 1 (max)", mode);
    U2_REQUIRE(nslab == u2mkd_scene_num_slabs(n, nb), "u2mkd_scene_pool_forward: nslab=%lld is not u2mkd_scene_num_slabs(n, nb)",
               (long long)nslab);
    if (n == 0 || nb == 0) return 0;
    U2_REQUIRE(x && order && seg && slab_seg && slabs && partial && out && (mode == 0 || arg), "u2mkd_scene_pool_forward: null pointer");
    U2_REQUIRE(gn_aligned16(x) && gn_aligned16(slabs) && gn_aligned16(partial),
               "u2mkd_scene_pool_forward: rows, the slab table and the workspace must be 16-byte aligned");
#define GN_CALL(T) \
    pool_forward_impl<T>(reinterpret_cast<const T *>(x), n, c, mode, order, seg, slab_seg, slabs, nslab, nb, partial, out, arg, s)
    return GN_BY_DTYPE(GN_CALL);
#undef GN_CALL
}

int u2mkd_scene_pool_backward(const float *dy, int32_t row_dtype, int64_t n, int32_t c, int32_t mode, const int32_t *bidx,
                              const int32_t *seg, const int32_t *arg, int64_t nb, void *dx, u2mkd_stream_t s) {
    GN_ROWS("u2mkd_scene_pool_backward");
    U2_REQUIRE(mode == 0 || mode == 1, "u2mkd_scene_pool_backward: mode %d must be 0 (mean) or 1 (max)", mode);
    if (n == 0) return 0;
    U2_REQUIRE(dx && (mode == 0 ? bidx && (nb == 0 || (dy && seg)) : nb == 0 || (dy && arg)), "u2mkd_scene_pool_backward: null pointer");
    U2_REQUIRE(gn_aligned16(dx) && gn_aligned16(dy), "u2mkd_scene_pool_backward: rows and dy must be 16-byte aligned");
#define GN_CALL(T) pool_backward_impl<T>(dy, n, c, mode, bidx, seg, arg, nb, reinterpret_cast<T *>(dx), s)
    return GN_BY_DTYPE(GN_CALL);
#undef GN_CALL
}

}  // extern "C"
