// BatchNorm over the rows of a [N, C] feature matrix, optionally fused with ReLU.
// Replaces spnn.BatchNorm + spnn.ReLU (= nn.BatchNorm1d / nn.ReLU applied to
// SparseTensor.feats through fapply; core/models/build_blocks.py:30-31,48-49,64-65,71,77;
// 49 instances per SPVCNN).
//
// HBM-bound row work.  Statistics are deterministic and cancellation-safe:
//   pass 1  each workgroup takes a slab of rows and computes, per channel, its local
//           mean and the centred second moment M2 around that mean (the slab is re-read
//           from L2), float4 columns x row lanes, the row lanes' sums added out of LDS;
//   pass 2  64 lanes per channel merge the slabs' (count, mean, M2) around a pivot that lies
//           among the data, in a fixed order (no atomics -> bitwise reproducible), write mean /
//           invstd and update the running statistics (unbiased variance, momentum) like
//           nn.BatchNorm1d;
//   pass 3  y = (x - mean) * invstd * gamma + beta [, ReLU]  (float4 elementwise).
// Backward mirrors it: slab partial sums of dy' and dy'*xhat (dy' = dy masked by the fused
// ReLU, recomputed from x), ordered merge, then
//   dx = gamma * invstd * (dy' - mean(dy') - xhat * mean(dy' * xhat)).
// ARITHMETIC.  Every sum over rows -- a slab's sum and second moment, the merge of the slabs and of the ranks, the gradient
// sums -- is carried in double and rounded once to the fp32 value that is stored (partials, mean, M2, dgamma, dbeta): the
// stored statistics are those of the rows to one fp32 rounding, whatever the mean and however many the rows (a channel that
// holds one value in every row has that value as its mean and M2 = 0, exactly).  The elementwise passes carry the arithmetic
// between a load and a store -- the normalise expression, the ReLU mask taken from it, the dx expression, the running update --
// in double and round once, as csrc/ln.hip does: in fp32 an element of dx passed six roundings and was up to 1.9 units in
// the last place off where torch's kernels were 0.8 off.  invstd is 1 / sqrt rounded once (bn_invstd).  Mean, invstd, M2 and
// the sums are read as the fp32 values stored.
// tests/row_bn_f64_ref.py bounds the same sequence carried out in fp32, which this is inside of.
#include "common.h"

#include <cstdlib>

namespace u2mkd {

constexpr int kBnThreads = 256;
constexpr int kBnSlabRows = 128;   // rows per workgroup in the partial passes (>= 600 workgroups at 80k rows)

// Rows are float, bf16 or fp16 (common.h: bf16row, _Float16, ld4, st4; the entries' row-dtype argument 0 / 1 / 2).  BF16 STORAGE (BASELINE.json configs[4]): under autocast the
// reference's BatchNorm1d takes and returns half rows with fp32 statistics; here bf16 rows, every sum, mean, invstd
// and gradient sum in fp32, one rounding per stored element.
// thread layout for a [rows, C4 float4] slab: j = float4 column, ry = row lane
struct BnLayout {
    int c4, rl;
};
__device__ __forceinline__ BnLayout bn_layout(int c) {
    BnLayout l;
    l.c4 = c >> 2;
    l.rl = kBnThreads / l.c4;
    if (l.rl < 1) l.rl = 1;
    return l;
}

// partial: [nslab][2][C] (mean_b, M2_b); rows of slab b = min(kBnSlabRows, n - b*kBnSlabRows)
// REG (c4 <= 32, i.e. C <= 128: at least 8 row lanes, at most 16 rows per thread): the thread's rows are loaded ONCE, all of
// them in flight together, and stay in registers for the second moment -- the same sums in the same order as the form
// below (bitwise the same partials), half the reads and no dependent load chain (the serial form: 12.5 us per launch on
// average in the KD step, 73 launches on the student's stream)
constexpr int kBnRegRows = 16;

// a float4 column's four sums in double (ARITHMETIC above)
struct BnAcc4 {
    double x, y, z, w;
};
__device__ __forceinline__ BnAcc4 bn_acc_zero() { return BnAcc4{0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ void bn_acc_add(BnAcc4 &a, const float4 &v) {
    a.x += (double)v.x; a.y += (double)v.y; a.z += (double)v.z; a.w += (double)v.w;
}
__device__ __forceinline__ void bn_acc_add(BnAcc4 &a, const BnAcc4 &v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
__device__ __forceinline__ void bn_acc_add_sq(BnAcc4 &a, const float4 &v, const BnAcc4 &m) {
    const double dx = (double)v.x - m.x, dy = (double)v.y - m.y, dz = (double)v.z - m.z, dw = (double)v.w - m.w;
    a.x += dx * dx; a.y += dy * dy; a.z += dz * dz; a.w += dw * dw;
}
// (bn_invstd, the one rounding of 1 / sqrt: common.h -- csrc/gn.hip takes its rstd from it too)
// running' = (1 - momentum) running + momentum s, from the stored (rounded) mean and M2, one rounding
__device__ __forceinline__ void bn_running_update(float *rm, float *rv, float momentum, float mean, double unbiased) {
    const double mo = (double)momentum;
    *rm = (float)((1.0 - mo) * (double)*rm + mo * (double)mean);
    *rv = (float)((1.0 - mo) * (double)*rv + mo * unbiased);
}
// the normalise expression: xhat = (x - mean) invstd and pre = xhat gamma + beta + res (res 0 without a residual)
__device__ __forceinline__ double bn_xhat(float v, float m, float is) { return ((double)v - (double)m) * (double)is; }
__device__ __forceinline__ double bn_pre(double h, float g, float b, float rv) { return h * (double)g + (double)b + (double)rv; }
__device__ __forceinline__ float bn_out(float v, float m, float is, float g, float b, float rv, int relu) {
    const double o = bn_pre(bn_xhat(v, m, is), g, b, rv);
    return (float)(relu ? fmax(o, 0.0) : o);
}
__device__ __forceinline__ float4 bn_acc_round(const BnAcc4 &a) { return make_float4((float)a.x, (float)a.y, (float)a.z, (float)a.w); }

template <typename T>
__global__ void __launch_bounds__(kBnThreads)
bn_stats_partial_reg_kernel(const T *__restrict__ x, int64_t n, int c, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) BnAcc4 red[];   // [rl][c4]
    const int c4 = c >> 2, rl = kBnThreads / c4;
    const int64_t r0 = (int64_t)blockIdx.x * kBnSlabRows;
    const int rows = (int)min((int64_t)kBnSlabRows, n - r0);
    const int j = threadIdx.x % c4, ry = threadIdx.x / c4;
    const bool live = ry < rl;
    float4 vals[kBnRegRows];
#pragma unroll
    for (int u = 0; u < kBnRegRows; ++u) {
        const int rr = ry + u * rl;
        vals[u] = (live && rr < rows) ? ld4(x, (r0 + rr) * c4 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    BnAcc4 s = bn_acc_zero();
#pragma unroll
    for (int u = 0; u < kBnRegRows; ++u)
        if (u * rl < rows) bn_acc_add(s, vals[u]);       // (the same for the whole workgroup; a row past the slab adds an exact zero)
    if (live) red[ry * c4 + j] = s;
    __syncthreads();
    // lane 0 of each column adds the row lanes' sums and hands the mean round (every lane adding all of them for itself
    // read rl x 256 entries out of LDS per workgroup)
    BnAcc4 mean = bn_acc_zero();
    if (live && ry == 0) {
        for (int g = 0; g < rl; ++g) bn_acc_add(mean, red[g * c4 + j]);
        const double inv = 1.0 / (double)rows;
        mean.x *= inv; mean.y *= inv; mean.z *= inv; mean.w *= inv;
    }
    __syncthreads();
    if (live && ry == 0) red[j] = mean;
    __syncthreads();
    if (live) mean = red[j];
    __syncthreads();
    BnAcc4 m2 = bn_acc_zero();
#pragma unroll
    for (int u = 0; u < kBnRegRows; ++u)
        if (live && ry + u * rl < rows) bn_acc_add_sq(m2, vals[u], mean);
    if (live) red[ry * c4 + j] = m2;
    __syncthreads();
    if (live && ry == 0) {
        BnAcc4 t = bn_acc_zero();
        for (int g = 0; g < rl; ++g) bn_acc_add(t, red[g * c4 + j]);
        float *p = partial + (size_t)blockIdx.x * 2 * c;
        *reinterpret_cast<float4 *>(p + 4 * j) = bn_acc_round(mean);
        *reinterpret_cast<float4 *>(p + c + 4 * j) = bn_acc_round(t);
    }
}

template <typename T>
__global__ void __launch_bounds__(kBnThreads)
bn_stats_partial_kernel(const T *__restrict__ x, int64_t n, int c, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) BnAcc4 red[];   // [rl][c4] (c4 <= 256)
    const int c4 = c >> 2;
    const int nloop = (c4 + kBnThreads - 1) / kBnThreads;           // > 1 only for C > 1024
    const int64_t r0 = (int64_t)blockIdx.x * kBnSlabRows;
    const int rows = (int)min((int64_t)kBnSlabRows, n - r0);
    for (int it = 0; it < nloop; ++it) {
        const int rl = c4 >= kBnThreads ? 1 : kBnThreads / c4;
        const int j = c4 >= kBnThreads ? it * kBnThreads + threadIdx.x : threadIdx.x % c4;
        const int ry = c4 >= kBnThreads ? 0 : threadIdx.x / c4;
        const bool live = j < c4 && ry < rl;
        BnAcc4 s = bn_acc_zero();
        if (live)
            for (int rr0 = ry; rr0 < rows; rr0 += 8 * rl) {       // (eight rows' loads in flight per trip, summed in row order)
                float4 vv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    vv[u] = rr0 + u * rl < rows ? ld4(x, (r0 + rr0 + u * rl) * c4 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < 8; ++u) bn_acc_add(s, vv[u]);
            }
        if (live) red[ry * c4 + (j % c4)] = s;
        __syncthreads();
        BnAcc4 mean = bn_acc_zero();
        if (live && ry == 0) {
            for (int g = 0; g < rl; ++g) bn_acc_add(mean, red[g * c4 + (j % c4)]);
            const double inv = 1.0 / (double)rows;
            mean.x *= inv; mean.y *= inv; mean.z *= inv; mean.w *= inv;
        }
        __syncthreads();
        if (live && ry == 0) red[j % c4] = mean;
        __syncthreads();
        if (live) mean = red[j % c4];
        __syncthreads();
        BnAcc4 m2 = bn_acc_zero();
        if (live)
            for (int rr0 = ry; rr0 < rows; rr0 += 8 * rl) {
                float4 vv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    vv[u] = rr0 + u * rl < rows ? ld4(x, (r0 + rr0 + u * rl) * c4 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (rr0 + u * rl >= rows) break;
                    bn_acc_add_sq(m2, vv[u], mean);
                }
            }
        if (live) red[ry * c4 + (j % c4)] = m2;
        __syncthreads();
        if (live && ry == 0) {
            BnAcc4 t = bn_acc_zero();
            for (int g = 0; g < rl; ++g) bn_acc_add(t, red[g * c4 + (j % c4)]);
            float *p = partial + (size_t)blockIdx.x * 2 * c;
            *reinterpret_cast<float4 *>(p + 4 * j) = bn_acc_round(mean);
            *reinterpret_cast<float4 *>(p + c + 4 * j) = bn_acc_round(t);
        }
        __syncthreads();
    }
}

// 4 channels x 64 slab lanes per block: lane g takes slabs g, g+64, ... (the loads of a lane's slabs are independent and
// issued four at a time -- with 16 lanes the 40 dependent round trips to L2 made this tiny kernel cost 10 us) and sums, in
// double, the slabs' counts, their means' weighted distances from a pivot K (slab 0's mean, which lies among the data:
// nothing large is subtracted) and their second moments around K; the 64 lanes' sums are added by a fixed binary tree
// through LDS, and mean = K + S / n, M2 = Q - S^2 / n.  No division on the way (Chan's update, two fp32 divisions per
// slab and per tree level, was what this kernel spent its time on), fixed order, no atomics: bitwise reproducible.
constexpr int kBnFinLanes = 64, kBnFinCh = 4;

__global__ void __launch_bounds__(256)
bn_stats_finalize_kernel(const float *__restrict__ partial, int nslab, int64_t n, int c, float eps,
                         float momentum, float *__restrict__ running_mean, float *__restrict__ running_var,
                         float *__restrict__ mean_out, float *__restrict__ invstd_out, float *__restrict__ m2_out,
                         int64_t *__restrict__ num_batches_tracked = nullptr, int slab_rows = kBnSlabRows) {
    // nn.BatchNorm's step counter (a separate one-element add_ launch per layer otherwise)
    if (num_batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *num_batches_tracked += 1;
    __shared__ double s_s[kBnFinLanes][kBnFinCh], s_q[kBnFinLanes][kBnFinCh];
    const int cl = threadIdx.x & (kBnFinCh - 1), g = threadIdx.x / kBnFinCh;
    const int ch = blockIdx.x * kBnFinCh + cl;
    const double pivot = ch < c ? (double)partial[ch] : 0.0;
    double ss = 0.0, qq = 0.0;
    if (ch < c) {
        for (int b0 = g; b0 < nslab; b0 += 4 * kBnFinLanes) {
            float mb[4], qb[4], nb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int b = b0 + u * kBnFinLanes;
                nb[u] = b < nslab ? (float)min((int64_t)slab_rows, n - (int64_t)b * slab_rows) : 0.f;
                mb[u] = b < nslab ? partial[(size_t)b * 2 * c + ch] : 0.f;
                qb[u] = b < nslab ? partial[(size_t)b * 2 * c + c + ch] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (nb[u] == 0.f) continue;
                const double w = (double)nb[u], d = (double)mb[u] - pivot;
                ss += w * d;
                qq += (double)qb[u] + w * d * d;
            }
        }
    }
    s_s[g][cl] = ss; s_q[g][cl] = qq;
    __syncthreads();
    for (int stride = kBnFinLanes / 2; stride >= 1; stride >>= 1) {
        if (g < stride) {
            s_s[g][cl] += s_s[g + stride][cl];
            s_q[g][cl] += s_q[g + stride][cl];
        }
        __syncthreads();
    }
    if (g != 0 || ch >= c) return;
    const double shift = s_s[0][cl] / (double)n;
    const double m2d = s_q[0][cl] - s_s[0][cl] * shift;
    // from here on in fp32, from the ROUNDED mean and M2: what u2mkd_bn_merge_stats computes from one rank's stats row
    const float mean = (float)(pivot + shift);
    const float m2 = m2d > 0.0 ? (float)m2d : 0.f;
    float var = m2 / (float)n;
    mean_out[ch] = mean;
    if (m2_out) {   // local statistics only (cross-rank merge follows): stats row = mean[c], M2[c], count
        m2_out[ch] = m2;
        if (ch == 0) m2_out[c] = (float)n;
        return;
    }
    invstd_out[ch] = bn_invstd((double)m2 / (double)n + (double)eps);
    if (running_mean) {
        const double unbiased = n > 1 ? (double)m2 / (double)(n - 1) : (double)var;
        bn_running_update(running_mean + ch, running_var + ch, momentum, mean, unbiased);
    }
}

// y = (x - mean) * invstd * gamma + beta [, relu]; gamma / beta may be null (affine=False)
// res (may be null): the residual branch of a ResidualBlock, y = relu(bn(x) + res) in the same pass
template <typename T>
__global__ void bn_apply_kernel(const T *__restrict__ x, int64_t total4, int c4, const float *__restrict__ mean,
                                const float *__restrict__ invstd, const float *__restrict__ gamma,
                                const float *__restrict__ beta, int relu, T *__restrict__ y,
                                const T *__restrict__ res = nullptr) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    int j = (int)(t % c4) * 4;
    float4 v = ld4(x, t);
    float4 m = *reinterpret_cast<const float4 *>(mean + j);
    float4 is = *reinterpret_cast<const float4 *>(invstd + j);
    float4 g = gamma ? *reinterpret_cast<const float4 *>(gamma + j) : make_float4(1.f, 1.f, 1.f, 1.f);
    float4 b = beta ? *reinterpret_cast<const float4 *>(beta + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 rv = res ? ld4(res, t) : make_float4(0.f, 0.f, 0.f, 0.f);
    st4(y, t, make_float4(bn_out(v.x, m.x, is.x, g.x, b.x, rv.x, relu), bn_out(v.y, m.y, is.y, g.y, b.y, rv.y, relu),
                          bn_out(v.z, m.z, is.z, g.z, b.z, rv.z, relu), bn_out(v.w, m.w, is.w, g.w, b.w, rv.w, relu)));
}

// eval mode: y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta [, relu] in ONE launch (the separate
// invstd pass was a launch per layer of the frozen KD teacher); workgroup 0 also writes invstd for a backward pass
template <typename T>
__global__ void bn_apply_eval_kernel(const T *__restrict__ x, int64_t total4, int c4, const float *__restrict__ mean,
                                     const float *__restrict__ var, float eps, const float *__restrict__ gamma,
                                     const float *__restrict__ beta, int relu, float *__restrict__ invstd_out,
                                     T *__restrict__ y, const T *__restrict__ res = nullptr) {
    if (blockIdx.x == 0 && invstd_out)
        for (int ch = threadIdx.x; ch < 4 * c4; ch += blockDim.x) invstd_out[ch] = bn_invstd((double)var[ch] + (double)eps);
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    int j = (int)(t % c4) * 4;
    float4 v = ld4(x, t);
    float4 m = *reinterpret_cast<const float4 *>(mean + j);
    float4 vr = *reinterpret_cast<const float4 *>(var + j);
    float4 is = make_float4(bn_invstd((double)vr.x + (double)eps), bn_invstd((double)vr.y + (double)eps), bn_invstd((double)vr.z + (double)eps),
                            bn_invstd((double)vr.w + (double)eps));
    float4 g = gamma ? *reinterpret_cast<const float4 *>(gamma + j) : make_float4(1.f, 1.f, 1.f, 1.f);
    float4 b = beta ? *reinterpret_cast<const float4 *>(beta + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 rv = res ? ld4(res, t) : make_float4(0.f, 0.f, 0.f, 0.f);
    st4(y, t, make_float4(bn_out(v.x, m.x, is.x, g.x, b.x, rv.x, relu), bn_out(v.y, m.y, is.y, g.y, b.y, rv.y, relu),
                          bn_out(v.z, m.z, is.z, g.z, b.z, rv.z, relu), bn_out(v.w, m.w, is.w, g.w, b.w, rv.w, relu)));
}

// partial: [nslab][2][C] (sum dy', sum dy' * xhat)
template <typename T>
__global__ void __launch_bounds__(kBnThreads)
bn_bwd_partial_kernel(const T *__restrict__ dy, const T *__restrict__ x, int64_t n, int c,
                      const float *__restrict__ mean, const float *__restrict__ invstd,
                      const float *__restrict__ gamma, const float *__restrict__ beta, int relu,
                      float *__restrict__ partial, const T *__restrict__ res = nullptr) {
    extern __shared__ __attribute__((aligned(16))) BnAcc4 red[];   // [2][rl][c4]
    const int c4 = c >> 2;
    const int nloop = (c4 + kBnThreads - 1) / kBnThreads;
    const int64_t r0 = (int64_t)blockIdx.x * kBnSlabRows;
    const int rows = (int)min((int64_t)kBnSlabRows, n - r0);
    for (int it = 0; it < nloop; ++it) {
        const int rl = c4 >= kBnThreads ? 1 : kBnThreads / c4;
        const int j = c4 >= kBnThreads ? it * kBnThreads + threadIdx.x : threadIdx.x % c4;
        const int ry = c4 >= kBnThreads ? 0 : threadIdx.x / c4;
        const bool live = j < c4 && ry < rl;
        const int cw = c4 >= kBnThreads ? kBnThreads : c4;
        const int jl = c4 >= kBnThreads ? threadIdx.x : j;
        BnAcc4 s1 = bn_acc_zero(), s2 = s1;
        if (live) {
            float4 m = *reinterpret_cast<const float4 *>(mean + 4 * j);
            float4 is = *reinterpret_cast<const float4 *>(invstd + 4 * j);
            float4 g = gamma ? *reinterpret_cast<const float4 *>(gamma + 4 * j) : make_float4(1.f, 1.f, 1.f, 1.f);
            float4 b = beta ? *reinterpret_cast<const float4 *>(beta + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            // four rows' loads in flight per trip (the sums in the same row order: bitwise the same partials)
            for (int rr0 = ry; rr0 < rows; rr0 += 4 * rl) {
                float4 vv[4], dd[4], rr4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int rr = rr0 + u * rl;
                    const bool ok = rr < rows;
                    vv[u] = ok ? ld4(x, (r0 + rr) * c4 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
                    dd[u] = ok ? ld4(dy, (r0 + rr) * c4 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
                    rr4[u] = (ok && relu && res) ? ld4(res, (r0 + rr) * c4 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (rr0 + u * rl >= rows) break;
                    const float4 v = vv[u], rv = rr4[u];
                    float4 d = dd[u];
                    const double hx = bn_xhat(v.x, m.x, is.x), hy = bn_xhat(v.y, m.y, is.y), hz = bn_xhat(v.z, m.z, is.z),
                                 hw = bn_xhat(v.w, m.w, is.w);
                    if (relu) {
                        if (bn_pre(hx, g.x, b.x, rv.x) <= 0.0) d.x = 0.f;
                        if (bn_pre(hy, g.y, b.y, rv.y) <= 0.0) d.y = 0.f;
                        if (bn_pre(hz, g.z, b.z, rv.z) <= 0.0) d.z = 0.f;
                        if (bn_pre(hw, g.w, b.w, rv.w) <= 0.0) d.w = 0.f;
                    }
                    bn_acc_add(s1, d);
                    s2.x += (double)d.x * hx; s2.y += (double)d.y * hy; s2.z += (double)d.z * hz; s2.w += (double)d.w * hw;
                }
            }
            red[ry * cw + jl] = s1;
            red[(rl + ry) * cw + jl] = s2;
        }
        __syncthreads();
        if (live && ry == 0) {
            BnAcc4 t1 = bn_acc_zero(), t2 = t1;
            for (int gq = 0; gq < rl; ++gq) {
                bn_acc_add(t1, red[gq * cw + jl]);
                bn_acc_add(t2, red[(rl + gq) * cw + jl]);
            }
            float *p = partial + (size_t)blockIdx.x * 2 * c;
            *reinterpret_cast<float4 *>(p + 4 * j) = bn_acc_round(t1);
            *reinterpret_cast<float4 *>(p + c + 4 * j) = bn_acc_round(t2);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
bn_bwd_finalize_kernel(const float *__restrict__ partial, int nslab, int c, float *__restrict__ dbeta,
                       float *__restrict__ dgamma, float *__restrict__ keep = nullptr) {
    __shared__ double s_1[kBnFinLanes][kBnFinCh], s_2[kBnFinLanes][kBnFinCh];
    const int cl = threadIdx.x & (kBnFinCh - 1), g = threadIdx.x / kBnFinCh;
    const int ch = blockIdx.x * kBnFinCh + cl;
    double s1 = 0.0, s2 = 0.0;
    if (ch < c) {
        for (int b0 = g; b0 < nslab; b0 += 4 * kBnFinLanes) {
            float p1[4], p2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int b = b0 + u * kBnFinLanes;
                p1[u] = b < nslab ? partial[(size_t)b * 2 * c + ch] : 0.f;
                p2[u] = b < nslab ? partial[(size_t)b * 2 * c + c + ch] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { s1 += (double)p1[u]; s2 += (double)p2[u]; }
        }
    }
    s_1[g][cl] = s1; s_2[g][cl] = s2;
    __syncthreads();
    for (int stride = kBnFinLanes / 2; stride >= 1; stride >>= 1) {      // (fixed binary tree over the 64 lanes)
        if (g < stride) {
            s_1[g][cl] += s_1[g + stride][cl];
            s_2[g][cl] += s_2[g + stride][cl];
        }
        __syncthreads();
    }
    if (g != 0 || ch >= c) return;
    const float f1 = (float)s_1[0][cl], f2 = (float)s_2[0][cl];
    dbeta[ch] = f1;
    dgamma[ch] = f2;
    if (keep) { keep[ch] = f1; keep[c + ch] = f2; }      // a second copy: the first one is summed over the ranks in place
}

template <typename T>
__global__ void bn_bwd_apply_kernel(const T *__restrict__ dy, const T *__restrict__ x, int64_t total4, int c4,
                                    double inv_n_host, const float *__restrict__ total_n,
                                    const float *__restrict__ mean, const float *__restrict__ invstd,
                                    const float *__restrict__ gamma, const float *__restrict__ beta, int relu,
                                    const float *__restrict__ dbeta, const float *__restrict__ dgamma,
                                    T *__restrict__ dx, const T *__restrict__ res = nullptr,
                                    T *__restrict__ dres = nullptr) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    const double inv_n = total_n ? 1.0 / (double)*total_n : inv_n_host;     // SyncBatchNorm: the count of all ranks
    int j = (int)(t % c4) * 4;
    float4 v = ld4(x, t);
    float4 d = ld4(dy, t);
    float4 m = *reinterpret_cast<const float4 *>(mean + j);
    float4 is = *reinterpret_cast<const float4 *>(invstd + j);
    float4 g = gamma ? *reinterpret_cast<const float4 *>(gamma + j) : make_float4(1.f, 1.f, 1.f, 1.f);
    float4 b = beta ? *reinterpret_cast<const float4 *>(beta + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 db = *reinterpret_cast<const float4 *>(dbeta + j);
    float4 dg = *reinterpret_cast<const float4 *>(dgamma + j);
    const double hx = bn_xhat(v.x, m.x, is.x), hy = bn_xhat(v.y, m.y, is.y), hz = bn_xhat(v.z, m.z, is.z), hw = bn_xhat(v.w, m.w, is.w);
    if (relu) {
        const float4 rv = res ? ld4(res, t) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (bn_pre(hx, g.x, b.x, rv.x) <= 0.0) d.x = 0.f;
        if (bn_pre(hy, g.y, b.y, rv.y) <= 0.0) d.y = 0.f;
        if (bn_pre(hz, g.z, b.z, rv.z) <= 0.0) d.z = 0.f;
        if (bn_pre(hw, g.w, b.w, rv.w) <= 0.0) d.w = 0.f;
    }
    if (dres) st4(dres, t, d);          // gradient of the residual branch = the masked dy
    float4 o;
    o.x = (float)((double)g.x * (double)is.x * ((double)d.x - (double)db.x * inv_n - hx * ((double)dg.x * inv_n)));
    o.y = (float)((double)g.y * (double)is.y * ((double)d.y - (double)db.y * inv_n - hy * ((double)dg.y * inv_n)));
    o.z = (float)((double)g.z * (double)is.z * ((double)d.z - (double)db.z * inv_n - hz * ((double)dg.z * inv_n)));
    o.w = (float)((double)g.w * (double)is.w * ((double)d.w - (double)db.w * inv_n - hw * ((double)dg.w * inv_n)));
    st4(dx, t, o);
}

// eval-mode backward / plain affine: dx = dy' * gamma * invstd
template <typename T>
__global__ void bn_bwd_eval_kernel(const T *__restrict__ dy, const T *__restrict__ x, int64_t total4, int c4,
                                   const float *__restrict__ mean, const float *__restrict__ invstd,
                                   const float *__restrict__ gamma, const float *__restrict__ beta, int relu,
                                   T *__restrict__ dx, const T *__restrict__ res = nullptr,
                                   T *__restrict__ dres = nullptr) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    int j = (int)(t % c4) * 4;
    float4 v = ld4(x, t);
    float4 d = ld4(dy, t);
    float4 m = *reinterpret_cast<const float4 *>(mean + j);
    float4 is = *reinterpret_cast<const float4 *>(invstd + j);
    float4 g = gamma ? *reinterpret_cast<const float4 *>(gamma + j) : make_float4(1.f, 1.f, 1.f, 1.f);
    float4 b = beta ? *reinterpret_cast<const float4 *>(beta + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (relu) {
        const float4 rv = res ? ld4(res, t) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (bn_pre(bn_xhat(v.x, m.x, is.x), g.x, b.x, rv.x) <= 0.0) d.x = 0.f;
        if (bn_pre(bn_xhat(v.y, m.y, is.y), g.y, b.y, rv.y) <= 0.0) d.y = 0.f;
        if (bn_pre(bn_xhat(v.z, m.z, is.z), g.z, b.z, rv.z) <= 0.0) d.z = 0.f;
        if (bn_pre(bn_xhat(v.w, m.w, is.w), g.w, b.w, rv.w) <= 0.0) d.w = 0.f;
    }
    if (dres) st4(dres, t, d);
    st4(dx, t, make_float4((float)((double)d.x * (double)g.x * (double)is.x), (float)((double)d.y * (double)g.y * (double)is.y),
                           (float)((double)d.z * (double)g.z * (double)is.z), (float)((double)d.w * (double)g.w * (double)is.w)));
}

__global__ void bn_invstd_kernel(const float *__restrict__ var, int c, float eps, float *__restrict__ invstd) {
    int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < c) invstd[ch] = bn_invstd((double)var[ch] + (double)eps);
}

// SyncBatchNorm: merge the per-rank (mean, M2, count) triples (rank order, Chan's update), write
// mean / invstd of the global batch and update the running statistics; stats rows are [2c+1].
__global__ void bn_sync_merge_kernel(const float *__restrict__ gathered, int world, int c, float eps, float momentum,
                                     float *__restrict__ running_mean, float *__restrict__ running_var,
                                     float *__restrict__ mean_out, float *__restrict__ invstd_out,
                                     float *__restrict__ total_out, int64_t *__restrict__ num_batches_tracked = nullptr) {
    int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (num_batches_tracked && ch == 0) *num_batches_tracked += 1;      // nn.BatchNorm's step counter (no launch of its own)
    if (ch >= c) return;
    const int row = 2 * c + 1;
    // (the update in double, the merged mean and M2 rounded once: with one rank they are that rank's own, bit for bit)
    double nad = 0.0, meand = 0.0, m2d = 0.0;
    for (int r = 0; r < world; ++r) {
        const double nb = (double)gathered[(size_t)r * row + 2 * c];
        if (nb == 0.0) continue;
        const double mb = (double)gathered[(size_t)r * row + ch], qb = (double)gathered[(size_t)r * row + c + ch];
        const double tot = nad + nb;
        const double delta = mb - meand;
        meand += delta * (nb / tot);
        m2d += qb + delta * delta * (nad * nb / tot);
        nad = tot;
    }
    const float na = (float)nad, mean = (float)meand, m2 = (float)m2d;
    float var = na > 0.f ? m2 / na : 0.f;
    mean_out[ch] = mean;
    invstd_out[ch] = bn_invstd((na > 0.f ? (double)m2 / (double)na : 0.0) + (double)eps);
    if (ch == 0) *total_out = na;
    if (running_mean) {
        const double unbiased = na > 1.f ? (double)m2 / ((double)na - 1.0) : (double)var;
        bn_running_update(running_mean + ch, running_var + ch, momentum, mean, unbiased);
    }
}

static size_t bn_lds_bytes(int c, int arrays) {
    int c4 = c / 4;
    int rl = c4 >= kBnThreads ? 1 : kBnThreads / c4;
    int cw = c4 >= kBnThreads ? kBnThreads : c4;
    return (size_t)arrays * rl * cw * sizeof(BnAcc4);
}

// ---- launch sequences, shared by the fp32-, bf16- and fp16-row entry points ------------------------------------
// U2MKD_BN_STATS_SERIAL=1: the statistics pass in its two-read form for every width (A/B; the partials are bitwise the same)
static bool bn_stats_serial() {
    static const bool on = [] { const char *e = getenv("U2MKD_BN_STATS_SERIAL"); return e && e[0] == '1'; }();
    return on;
}

template <typename T>
static void bn_launch_stats_partial(hipStream_t st, int nslab, const T *x, int64_t n, int c, float *partial) {
    const int c4 = c / 4;
    if (c4 <= 32 && kBnSlabRows / (kBnThreads / c4) <= kBnRegRows && !bn_stats_serial())
        hipLaunchKernelGGL(bn_stats_partial_reg_kernel<T>, dim3(nslab), dim3(kBnThreads), bn_lds_bytes(c, 1), st, x, n, c, partial);
    else
        hipLaunchKernelGGL(bn_stats_partial_kernel<T>, dim3(nslab), dim3(kBnThreads), bn_lds_bytes(c, 1), st, x, n, c, partial);
}

template <typename T>
static int bn_train_forward_impl(const T *x, const T *res, int64_t n, int32_t c, const float *gamma, const float *beta,
                                 float eps, float momentum, float *running_mean, float *running_var,
                                 int64_t *num_batches_tracked, int32_t relu, float *partial, float *mean, float *invstd, T *y,
                                 u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0 && c <= 1024, "u2mkd_bn_train_forward: c=%d must be a multiple of 4 in 4..1024", c);
    U2_REQUIRE(n > 0, "u2mkd_bn_train_forward: empty batch (n=%lld)", (long long)n);
    U2_REQUIRE(x && partial && mean && invstd && y, "u2mkd_bn_train_forward: null pointer");
    hipStream_t st = as_stream(s);
    int nslab = (int)u2mkd_bn_num_slabs(n);
#ifndef U2MKD_EXP_SKIP_BN_STATS      // (tools/build_variant.sh: an UPPER BOUND on what statistics taken in the producer's store could buy)
    bn_launch_stats_partial<T>(st, nslab, x, n, c, partial);
#endif
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((unsigned)ceil_div(c, kBnFinCh)), dim3(256), 0, st, partial, nslab, n, c,
                       eps, momentum, running_mean, running_var, mean, invstd, (float *)nullptr, num_batches_tracked);
    int64_t total4 = n * (c / 4);
    hipLaunchKernelGGL(bn_apply_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, x, total4, c / 4, mean,
                       invstd, gamma, beta, relu, y, res);
    return check_launch("u2mkd_bn_train_forward");
}

// train-mode forward from slab partials somebody else computed (the gather-sum of the producing convolution:
// u2mkd_pairs_gather_sum_stats, slabs of `slab_rows` rows): merge + apply
static int bn_train_forward_from_partial_impl(const float *x, const float *res, int64_t n, int32_t c, const float *gamma,
                                              const float *beta, float eps, float momentum, float *running_mean,
                                              float *running_var, int64_t *num_batches_tracked, int32_t relu,
                                              const float *partial, int32_t slab_rows, float *mean, float *invstd, float *y,
                                              u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0 && c <= 1024, "u2mkd_bn_train_forward_from_partial: c=%d must be a multiple of 4 in 4..1024", c);
    U2_REQUIRE(n > 0 && slab_rows > 0, "u2mkd_bn_train_forward_from_partial: n=%lld rows in slabs of %d", (long long)n, slab_rows);
    U2_REQUIRE(x && partial && mean && invstd && y, "u2mkd_bn_train_forward_from_partial: null pointer");
    U2_REQUIRE(res == nullptr || relu, "u2mkd_bn_train_forward_from_partial: a residual input is only fused with the ReLU form");
    hipStream_t st = as_stream(s);
    const int64_t nslab = ceil_div(n, (int64_t)slab_rows);
    U2_REQUIRE(nslab < ((int64_t)1 << 31), "u2mkd_bn_train_forward_from_partial: too many slabs");
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((unsigned)ceil_div(c, kBnFinCh)), dim3(256), 0, st, partial, (int)nslab, n, c,
                       eps, momentum, running_mean, running_var, mean, invstd, (float *)nullptr, num_batches_tracked, (int)slab_rows);
    int64_t total4 = n * (c / 4);
    hipLaunchKernelGGL(bn_apply_kernel<float>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, x, total4, c / 4, mean,
                       invstd, gamma, beta, relu, y, res);
    return check_launch("u2mkd_bn_train_forward_from_partial");
}

template <typename T>
static int bn_eval_forward_impl(const T *x, const T *res, int64_t n, int32_t c, const float *gamma, const float *beta,
                                float eps, const float *running_mean, const float *running_var, int32_t relu, float *invstd,
                                T *y, u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0, "u2mkd_bn_eval_forward: c=%d must be a positive multiple of 4", c);
    if (n == 0) return 0;
    U2_REQUIRE(x && running_mean && running_var && invstd && y, "u2mkd_bn_eval_forward: null pointer");
    hipStream_t st = as_stream(s);
    int64_t total4 = n * (c / 4);
    hipLaunchKernelGGL(bn_apply_eval_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, x, total4, c / 4,
                       running_mean, running_var, eps, gamma, beta, relu, invstd, y, res);
    return check_launch("u2mkd_bn_eval_forward");
}

template <typename T>
static int bn_backward_impl(const T *dy, const T *x, const T *res, int64_t n, int32_t c, const float *mean,
                            const float *invstd, const float *gamma, const float *beta, int32_t relu, int32_t training,
                            float *partial, float *dgamma, float *dbeta, T *dx, T *dres, u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0 && c <= 1024, "u2mkd_bn_backward: c=%d must be a multiple of 4 in 4..1024", c);
    U2_REQUIRE((res == nullptr) == (dres == nullptr), "u2mkd_bn_backward: res and dres go together");
    U2_REQUIRE(res == nullptr || relu, "u2mkd_bn_backward: a residual input is only fused with the ReLU form");
    if (n == 0) return 0;
    U2_REQUIRE(dy && x && mean && invstd && partial && dgamma && dbeta && dx, "u2mkd_bn_backward: null pointer");
    hipStream_t st = as_stream(s);
    int nslab = (int)u2mkd_bn_num_slabs(n);
    hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, dim3(nslab), dim3(kBnThreads), bn_lds_bytes(c, 2), st, dy, x, n, c, mean,
                       invstd, gamma, beta, relu, partial, res);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)ceil_div(c, kBnFinCh)), dim3(256), 0, st, partial, nslab, c,
                       dbeta, dgamma);
    int64_t total4 = n * (c / 4);
    if (training)
        hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, dy, x, total4,
                           c / 4, 1.0 / (double)n, (const float *)nullptr, mean, invstd, gamma, beta, relu, dbeta, dgamma,
                           dx, res, dres);
    else
        hipLaunchKernelGGL(bn_bwd_eval_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, dy, x, total4,
                           c / 4, mean, invstd, gamma, beta, relu, dx, res, dres);
    return check_launch("u2mkd_bn_backward");
}

template <typename T>
static int bn_local_stats_impl(const T *x, int64_t n, int32_t c, float *partial, float *stats, u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0 && c <= 1024, "u2mkd_bn_local_stats: c=%d must be a multiple of 4 in 4..1024", c);
    U2_REQUIRE(stats && (n == 0 || (x && partial)), "u2mkd_bn_local_stats: null pointer");
    hipStream_t st = as_stream(s);
    if (n == 0) {
        (void)hipMemsetAsync(stats, 0, (size_t)(2 * c + 1) * sizeof(float), st);
        return check_launch("u2mkd_bn_local_stats");
    }
    int nslab = (int)u2mkd_bn_num_slabs(n);
    bn_launch_stats_partial<T>(st, nslab, x, n, c, partial);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((unsigned)ceil_div(c, kBnFinCh)), dim3(256), 0, st, partial, nslab,
                       n, c, 0.f, 0.f, (float *)nullptr, (float *)nullptr, stats, (float *)nullptr, stats + c);
    return check_launch("u2mkd_bn_local_stats");
}

template <typename T>
static int bn_apply_impl(const T *x, const T *res, int64_t n, int32_t c, const float *mean, const float *invstd,
                         const float *gamma, const float *beta, int32_t relu, T *y, u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0, "u2mkd_bn_apply: c=%d must be a positive multiple of 4", c);
    if (n == 0) return 0;
    U2_REQUIRE(x && mean && invstd && y, "u2mkd_bn_apply: null pointer");
    int64_t total4 = n * (c / 4);
    hipLaunchKernelGGL(bn_apply_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, as_stream(s), x, total4,
                       c / 4, mean, invstd, gamma, beta, relu, y, res);
    return check_launch("u2mkd_bn_apply");
}

template <typename T>
static int bn_backward_local_impl(const T *dy, const T *x, const T *res, int64_t n, int32_t c, const float *mean,
                                  const float *invstd, const float *gamma, const float *beta, int32_t relu, float *partial,
                                  float *sums, float *keep, u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0 && c <= 1024, "u2mkd_bn_backward_local: c=%d must be a multiple of 4 in 4..1024", c);
    U2_REQUIRE(sums, "u2mkd_bn_backward_local: null pointer");
    hipStream_t st = as_stream(s);
    if (n == 0) {
        (void)hipMemsetAsync(sums, 0, (size_t)2 * c * sizeof(float), st);
        if (keep) (void)hipMemsetAsync(keep, 0, (size_t)2 * c * sizeof(float), st);
        return check_launch("u2mkd_bn_backward_local");
    }
    U2_REQUIRE(dy && x && mean && invstd && partial, "u2mkd_bn_backward_local: null pointer");
    int nslab = (int)u2mkd_bn_num_slabs(n);
    hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, dim3(nslab), dim3(kBnThreads), bn_lds_bytes(c, 2), st, dy, x, n, c, mean,
                       invstd, gamma, beta, relu, partial, res);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)ceil_div(c, kBnFinCh)), dim3(256), 0, st, partial, nslab, c,
                       sums, sums + c, keep);
    return check_launch("u2mkd_bn_backward_local");
}

template <typename T>
static int bn_backward_apply_impl(const T *dy, const T *x, const T *res, int64_t n, int32_t c, const float *total_n,
                                  const float *mean, const float *invstd, const float *gamma, const float *beta, int32_t relu,
                                  const float *sums, T *dx, T *dres, u2mkd_stream_t s) {
    U2_REQUIRE(c > 0 && c % 4 == 0, "u2mkd_bn_backward_apply: c=%d must be a positive multiple of 4", c);
    if (n == 0) return 0;
    U2_REQUIRE(dy && x && total_n && mean && invstd && sums && dx, "u2mkd_bn_backward_apply: null pointer");
    int64_t total4 = n * (c / 4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, as_stream(s), dy, x,
                       total4, c / 4, 0.0, total_n, mean, invstd, gamma, beta, relu, sums, sums + c, dx, res, dres);
    return check_launch("u2mkd_bn_backward_apply");
}

}  // namespace u2mkd

using namespace u2mkd;

// the row pointers of the entries below as the rows of one dtype
#define BF(p) reinterpret_cast<const bf16row *>(p)
#define BFW(p) reinterpret_cast<bf16row *>(p)
#define H16(p) reinterpret_cast<const _Float16 *>(p)
#define H16W(p) reinterpret_cast<_Float16 *>(p)
// the row-dtype argument: 0 = fp32, 1 = bf16, 2 = fp16; anything else is an error
#define U2_ROW_DTYPE(who) U2_REQUIRE(row_dtype >= 0 && row_dtype <= 2, who ": row dtype %d must be 0 (fp32), 1 (bf16) or 2 (fp16)", row_dtype)
#define F32(p) reinterpret_cast<const float *>(p)
#define F32W(p) reinterpret_cast<float *>(p)

extern "C" {

int64_t u2mkd_bn_num_slabs(int64_t n) { return n > 0 ? (n + kBnSlabRows - 1) / kBnSlabRows : 0; }

int u2mkd_bn_train_forward(const void *x, const void *res, int32_t row_dtype, int64_t n, int32_t c, const float *gamma,
                           const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                           int64_t *num_batches_tracked, int32_t relu, float *partial, float *mean, float *invstd, void *y,
                           u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_bn_train_forward");
    if (row_dtype == 2)
        return bn_train_forward_impl<_Float16>(H16(x), H16(res), n, c, gamma, beta, eps, momentum, running_mean, running_var,
                                              num_batches_tracked, relu, partial, mean, invstd, H16W(y), s);
    if (row_dtype == 1)
        return bn_train_forward_impl<bf16row>(BF(x), BF(res), n, c, gamma, beta, eps, momentum, running_mean, running_var,
                                              num_batches_tracked, relu, partial, mean, invstd, BFW(y), s);
    return bn_train_forward_impl<float>(F32(x), F32(res), n, c, gamma, beta, eps, momentum, running_mean, running_var,
                                        num_batches_tracked, relu, partial, mean, invstd, F32W(y), s);
}

int u2mkd_bn_train_forward_from_partial(const float *x, const float *res, int64_t n, int32_t c, const float *gamma,
                                        const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                                        int64_t *num_batches_tracked, int32_t relu, const float *partial, int32_t slab_rows,
                                        float *mean, float *invstd, float *y, u2mkd_stream_t s) {
    return bn_train_forward_from_partial_impl(x, res, n, c, gamma, beta, eps, momentum, running_mean, running_var,
                                              num_batches_tracked, relu, partial, slab_rows, mean, invstd, y, s);
}

int u2mkd_bn_eval_forward(const void *x, const void *res, int32_t row_dtype, int64_t n, int32_t c, const float *gamma,
                          const float *beta, float eps, const float *running_mean, const float *running_var, int32_t relu,
                          float *invstd, void *y, u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_bn_eval_forward");
    if (row_dtype == 2)
        return bn_eval_forward_impl<_Float16>(H16(x), H16(res), n, c, gamma, beta, eps, running_mean, running_var, relu, invstd,
                                             H16W(y), s);
    if (row_dtype == 1)
        return bn_eval_forward_impl<bf16row>(BF(x), BF(res), n, c, gamma, beta, eps, running_mean, running_var, relu, invstd,
                                             BFW(y), s);
    return bn_eval_forward_impl<float>(F32(x), F32(res), n, c, gamma, beta, eps, running_mean, running_var, relu, invstd,
                                       F32W(y), s);
}

int u2mkd_bn_backward(const void *dy, const void *x, const void *res, int32_t row_dtype, int64_t n, int32_t c,
                      const float *mean, const float *invstd, const float *gamma, const float *beta, int32_t relu,
                      int32_t training, float *partial, float *dgamma, float *dbeta, void *dx, void *dres, u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_bn_backward");
    if (row_dtype == 2)
        return bn_backward_impl<_Float16>(H16(dy), H16(x), H16(res), n, c, mean, invstd, gamma, beta, relu, training, partial,
                                         dgamma, dbeta, H16W(dx), H16W(dres), s);
    if (row_dtype == 1)
        return bn_backward_impl<bf16row>(BF(dy), BF(x), BF(res), n, c, mean, invstd, gamma, beta, relu, training, partial,
                                         dgamma, dbeta, BFW(dx), BFW(dres), s);
    return bn_backward_impl<float>(F32(dy), F32(x), F32(res), n, c, mean, invstd, gamma, beta, relu, training, partial, dgamma,
                                   dbeta, F32W(dx), F32W(dres), s);
}

/* ---- SyncBatchNorm pieces: local statistics | (all_gather by the caller) | merge | apply, and
 * local sums | (all_reduce by the caller) | apply in the backward ---- */
int u2mkd_bn_local_stats(const void *x, int32_t row_dtype, int64_t n, int32_t c, float *partial, float *stats,
                         u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_bn_local_stats");
    if (row_dtype == 2) return bn_local_stats_impl<_Float16>(H16(x), n, c, partial, stats, s);
    if (row_dtype == 1) return bn_local_stats_impl<bf16row>(BF(x), n, c, partial, stats, s);
    return bn_local_stats_impl<float>(F32(x), n, c, partial, stats, s);
}

int u2mkd_bn_merge_stats(const float *gathered, int32_t world, int32_t c, float eps, float momentum, float *running_mean,
                         float *running_var, float *mean, float *invstd, float *total, int64_t *num_batches_tracked,
                         u2mkd_stream_t s) {
    U2_REQUIRE(gathered && mean && invstd && total && world > 0 && c > 0, "u2mkd_bn_merge_stats: bad arguments");
    hipLaunchKernelGGL(bn_sync_merge_kernel, dim3((unsigned)ceil_div(c, 64)), dim3(64), 0, as_stream(s), gathered, world, c,
                       eps, momentum, running_mean, running_var, mean, invstd, total, num_batches_tracked);
    return check_launch("u2mkd_bn_merge_stats");
}

int u2mkd_bn_apply(const void *x, const void *res, int32_t row_dtype, int64_t n, int32_t c, const float *mean,
                   const float *invstd, const float *gamma, const float *beta, int32_t relu, void *y, u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_bn_apply");
    if (row_dtype == 2) return bn_apply_impl<_Float16>(H16(x), H16(res), n, c, mean, invstd, gamma, beta, relu, H16W(y), s);
    if (row_dtype == 1) return bn_apply_impl<bf16row>(BF(x), BF(res), n, c, mean, invstd, gamma, beta, relu, BFW(y), s);
    return bn_apply_impl<float>(F32(x), F32(res), n, c, mean, invstd, gamma, beta, relu, F32W(y), s);
}

int u2mkd_bn_backward_local(const void *dy, const void *x, const void *res, int32_t row_dtype, int64_t n, int32_t c,
                            const float *mean, const float *invstd, const float *gamma, const float *beta, int32_t relu,
                            float *partial, float *sums, float *keep, u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_bn_backward_local");
    if (row_dtype == 2)
        return bn_backward_local_impl<_Float16>(H16(dy), H16(x), H16(res), n, c, mean, invstd, gamma, beta, relu, partial, sums,
                                               keep, s);
    if (row_dtype == 1)
        return bn_backward_local_impl<bf16row>(BF(dy), BF(x), BF(res), n, c, mean, invstd, gamma, beta, relu, partial, sums,
                                               keep, s);
    return bn_backward_local_impl<float>(F32(dy), F32(x), F32(res), n, c, mean, invstd, gamma, beta, relu, partial, sums, keep,
                                         s);
}

int u2mkd_bn_backward_apply(const void *dy, const void *x, const void *res, int32_t row_dtype, int64_t n, int32_t c,
                            const float *total_n, const float *mean, const float *invstd, const float *gamma,
                            const float *beta, int32_t relu, const float *sums, void *dx, void *dres, u2mkd_stream_t s) {
    U2_ROW_DTYPE("u2mkd_bn_backward_apply");
    if (row_dtype == 2)
        return bn_backward_apply_impl<_Float16>(H16(dy), H16(x), H16(res), n, c, total_n, mean, invstd, gamma, beta, relu, sums,
                                               H16W(dx), H16W(dres), s);
    if (row_dtype == 1)
        return bn_backward_apply_impl<bf16row>(BF(dy), BF(x), BF(res), n, c, total_n, mean, invstd, gamma, beta, relu, sums,
                                               BFW(dx), BFW(dres), s);
    return bn_backward_apply_impl<float>(F32(dy), F32(x), F32(res), n, c, total_n, mean, invstd, gamma, beta, relu, sums,
                                         F32W(dx), F32W(dres), s);
}

}  // extern "C"
