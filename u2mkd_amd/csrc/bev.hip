// Bird's-eye-view operators of torchsparse.nn (ToBEVReduction, ToBEVConvolution, ToDenseBEVConvolution,
// ToBEVHeightCompression): the plan kernel over the coordinates, the neighbour tables of the "height is the offset"
// convolution, the segment mean in double, and the dense NCHW store / gather through a transposed LDS tile.
// The C ABI and the semantics are in include/u2mkd_hip.h.
#include "common.h"

namespace u2mkd {

// ---- the plan ---------------------------------------------------------------------------------------------------------------
struct BevGeom {
    int dim, b0, b1;        // the height axis and the two BEV axes (ascending)
    int mode, hmode;
    int s[3];               // tensor stride
    int a[3];               // mode 0: the cell quantum per axis (trunc(c / a) * a); mode 1: the offset per axis
    int h, w, nz;
};

__global__ __launch_bounds__(256) void bev_plan_kernel(const int4 *__restrict__ coords, int64_t n, BevGeom g,
                                                       int64_t *__restrict__ keys, int32_t *__restrict__ hidx,
                                                       int32_t *__restrict__ block) {
    __shared__ int s_bad[256];
    __shared__ int s_nb[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int bad = 0, nb = 0;
    if (i < n) {
        const int4 c4 = coords[i];
        const int c[3] = {c4.x, c4.y, c4.z};
        const int b = c4.w;
        nb = b >= 0 ? b + 1 : 0;
        int hz = 0;
        if (g.hmode == 1) {                     // the kernel index: trunc(c / s), checked, the offset NOT subtracted
            hz = c[g.dim] / g.s[g.dim];
            if (hz < 0 || hz >= g.nz) { bad = 1; hz = 0; }
        } else if (g.hmode == 2) {              // the height slot: trunc((c - offset) / s) clamped to 0..nz-1
            hz = (int)(((int64_t)c[g.dim] - g.a[g.dim]) / g.s[g.dim]);
            hz = hz < 0 ? 0 : (hz >= g.nz ? g.nz - 1 : hz);
        }
        int64_t key;
        if (g.mode == 0) {
            int o[3];
            o[g.dim] = 0;
            o[g.b0] = c[g.b0] / g.a[g.b0] * g.a[g.b0];
            o[g.b1] = c[g.b1] / g.a[g.b1] * g.a[g.b1];
            const int lim = 1 << 17;
            const bool ok = b >= 0 && b < 512 && o[0] > -lim - 1 && o[0] < lim && o[1] > -lim - 1 && o[1] < lim && o[2] > -lim - 1 && o[2] < lim;
            const int64_t bias = 1 << 17;
            key = ok ? (((int64_t)b << 54) | ((o[0] + bias) << 36) | ((o[1] + bias) << 18) | (o[2] + bias)) : INT64_MAX;
            if (!ok) bad = 1;
        } else {
            const int64_t u = ((int64_t)c[g.b0] - g.a[g.b0]) / g.s[g.b0];
            const int64_t v = ((int64_t)c[g.b1] - g.a[g.b1]) / g.s[g.b1];
            const bool ok = b >= 0 && u >= 0 && u < g.h && v >= 0 && v < g.w;
            key = ok ? ((int64_t)b * g.h + u) * g.w + v : -1;
            if (!ok) bad = 1;
        }
        keys[i] = key;
        hidx[i] = hz;
    }
    s_bad[threadIdx.x] = bad;
    s_nb[threadIdx.x] = nb;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s_bad[threadIdx.x] += s_bad[threadIdx.x + d];
            s_nb[threadIdx.x] = max(s_nb[threadIdx.x], s_nb[threadIdx.x + d]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {                     // the flag / count block: one update per workgroup
        if (s_bad[0]) atomicAdd(block + 0, s_bad[0]);
        if (s_nb[0]) atomicMax(block + 1, s_nb[0]);
    }
}

// nbr [nk, n_out] = -1 everywhere; nbr_inv [nk, n_in]: row r has exactly one offset, hidx[r], and feeds group[r] through it
__global__ void bev_tables_fill_kernel(const int32_t *__restrict__ group, const int32_t *__restrict__ hidx, int64_t n_in,
                                       int64_t n_out, int nk, int32_t *__restrict__ nbr, int32_t *__restrict__ nbr_inv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nk * n_out) nbr[i] = -1;
    if (i < nk * n_in) {
        const int64_t k = i / n_in, r = i - k * n_in;
        nbr_inv[i] = hidx[r] == (int)k ? group[r] : -1;
    }
}

// nbr[hidx[r]][group[r]] = r: a (group, height) pair holds at most one row, so every slot has one writer
__global__ void bev_tables_rows_kernel(const int32_t *__restrict__ group, const int32_t *__restrict__ hidx, int64_t n_in,
                                       int64_t n_out, int nk, int32_t *__restrict__ nbr) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_in) return;
    const int h = hidx[r], g = group[r];
    if (h >= 0 && h < nk && g >= 0 && g < n_out) nbr[(int64_t)h * n_out + g] = (int32_t)r;
}

// ---- the mean of the rows of a segment, summed in double and rounded once -----------------------------------------------
template <typename T>
__global__ void bev_segment_mean_kernel(const T *__restrict__ src, int c4, int64_t n_src, const int32_t *__restrict__ order,
                                        const int32_t *__restrict__ seg, int64_t nv, T *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t v = t / c4;
    if (v >= nv) return;
    const int j = (int)(t - v * c4);
    const int e0 = seg[v], e1 = seg[v + 1];
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    for (int e = e0; e < e1; ++e) {
        const int64_t r = order[e];
        if (r < 0 || r >= n_src) continue;
        const float4 f = ld4<T>(src, r * c4 + j);
        a0 += f.x; a1 += f.y; a2 += f.z; a3 += f.w;
    }
    const double m = e1 > e0 ? (double)(e1 - e0) : 1.;
    st4<T>(out, t, make_float4((float)(a0 / m), (float)(a1 / m), (float)(a2 / m), (float)(a3 / m)));
}

// ---- dense store and gather -------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float ld1(const T *p, int64_t i);
template <> __device__ __forceinline__ float ld1<float>(const float *p, int64_t i) { return p[i]; }
template <> __device__ __forceinline__ float ld1<bf16row>(const bf16row *p, int64_t i) { return __uint_as_float((uint32_t)p[i].v << 16); }
template <> __device__ __forceinline__ float ld1<_Float16>(const _Float16 *p, int64_t i) { return (float)p[i]; }
template <typename T> __device__ __forceinline__ void st1(T *p, int64_t i, float v);
template <> __device__ __forceinline__ void st1<float>(float *p, int64_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void st1<bf16row>(bf16row *p, int64_t i, float v) {
    const __bf16 a = (__bf16)v;
    p[i].v = __builtin_bit_cast(unsigned short, a);
}
template <> __device__ __forceinline__ void st1<_Float16>(_Float16 *p, int64_t i, float v) { p[i] = (_Float16)v; }

constexpr int kBevCells = 64;       // cells (consecutive positions u * W + v of one batch index) a workgroup owns
constexpr int kBevTile = 128;       // most channels of the result in one LDS tile (z > 1)
constexpr int kBevTile1 = 32;       // ... where the rows are the cells (z = 1): more, smaller workgroups (NOTES N24.3)

// out [nb, c * z, hw] (NCHW, hw = h * w) from rows src [n_rows, c]: out[b][ch * z + q][p] = the fp32 sum, in ascending entry
// order, of src[order[e]][ch] over the entries e of slot (b * hw + p) * z + q (seg == NULL: z = 1 and the row IS the slot).
// A workgroup owns 64 cells of one batch index and one chunk of cc channels (grid z): rows are read 16 bytes per lane along
// their channels into the tile [cell][channel] (row stride tch + 1 floats, odd), the tile is read back cell-fastest and every
// element of the result is stored once, 64 consecutive positions per wave.
template <typename T>
__global__ __launch_bounds__(256) void bev_dense_store_kernel(const T *__restrict__ src, int64_t n_rows, int c, const int32_t *__restrict__ seg,
                                                              const int32_t *__restrict__ order, int z, int cc, int64_t hw,
                                                              T *__restrict__ out) {
    extern __shared__ float tile[];
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kBevCells;
    const int ncell = (int)min((int64_t)kBevCells, hw - p0);
    const int ldw = cc * z + 1;
    const int c4 = c / 4;
    const int64_t cz = (int64_t)c * z;
    {
        const int c0 = blockIdx.z * cc;
        const int cur = min(cc, c - c0), q4 = cur / 4;
        const int items = ncell * z * q4;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int j = i % q4, q = (i / q4) % z, cell = i / (q4 * z);
            const int64_t slot = ((int64_t)b * hw + p0 + cell) * z + q;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (seg) {
                const int e0 = seg[slot], e1 = seg[slot + 1];
                bool first = true;
                for (int e = e0; e < e1; ++e) {
                    const int64_t r = order[e];
                    if (r < 0 || r >= n_rows) continue;
                    const float4 f = ld4<T>(src, r * c4 + c0 / 4 + j);
                    if (first) { acc = f; first = false; }
                    else { acc.x += f.x; acc.y += f.y; acc.z += f.z; acc.w += f.w; }
                }
            } else if (slot < n_rows) {
                acc = ld4<T>(src, slot * c4 + c0 / 4 + j);
            }
            float *t = tile + cell * ldw + (4 * j) * z + q;
            t[0] = acc.x; t[z] = acc.y; t[2 * z] = acc.z; t[3 * z] = acc.w;
        }
        __syncthreads();
        const int chans = cur * z;
        for (int i = threadIdx.x; i < chans * kBevCells; i += 256) {
            const int cell = i & (kBevCells - 1), ch = i >> 6;
            if (cell < ncell) st1<T>(out, ((int64_t)b * cz + (int64_t)c0 * z + ch) * hw + p0 + cell, tile[cell * ldw + ch]);
        }
    }
}

// the other direction: dsrc[r][ch] = dout[b][ch * z + q][p] for every row r of slot (b, p, q) -- rows that share a slot all read it
template <typename T>
__global__ __launch_bounds__(256) void bev_dense_gather_kernel(const T *__restrict__ dout, int64_t n_rows, int c, const int32_t *__restrict__ seg,
                                                               const int32_t *__restrict__ order, int z, int cc, int64_t hw,
                                                               T *__restrict__ dsrc) {
    extern __shared__ float tile[];
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kBevCells;
    const int ncell = (int)min((int64_t)kBevCells, hw - p0);
    const int ldw = cc * z + 1;
    const int c4 = c / 4;
    const int64_t cz = (int64_t)c * z;
    {
        const int c0 = blockIdx.z * cc;
        const int cur = min(cc, c - c0), q4 = cur / 4;
        const int chans = cur * z;
        for (int i = threadIdx.x; i < chans * kBevCells; i += 256) {
            const int cell = i & (kBevCells - 1), ch = i >> 6;
            tile[cell * ldw + ch] = cell < ncell ? ld1<T>(dout, ((int64_t)b * cz + (int64_t)c0 * z + ch) * hw + p0 + cell) : 0.f;
        }
        __syncthreads();
        const int items = ncell * z * q4;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int j = i % q4, q = (i / q4) % z, cell = i / (q4 * z);
            const int64_t slot = ((int64_t)b * hw + p0 + cell) * z + q;
            const float *t = tile + cell * ldw + (4 * j) * z + q;
            const float4 g = make_float4(t[0], t[z], t[2 * z], t[3 * z]);
            if (seg) {
                const int e0 = seg[slot], e1 = seg[slot + 1];
                for (int e = e0; e < e1; ++e) {
                    const int64_t r = order[e];
                    if (r >= 0 && r < n_rows) st4<T>(dsrc, r * c4 + c0 / 4 + j, g);
                }
            } else if (slot < n_rows) {
                st4<T>(dsrc, slot * c4 + c0 / 4 + j, g);
            }
        }
    }
}

static int bev_chunk(int c, int z) { return min(c, z == 1 ? kBevTile1 : (kBevTile / z) & ~3); }

template <typename T>
static int bev_dense_launch(bool store, const void *a, int64_t n_rows, int c, const int32_t *seg, const int32_t *order, int64_t nb,
                            int z, int64_t hw, void *o, u2mkd_stream_t s) {
    const int cc = bev_chunk(c, z);
    const size_t lds = (size_t)kBevCells * (cc * z + 1) * sizeof(float);
    const dim3 grid((unsigned)ceil_div(hw, kBevCells), (unsigned)nb, (unsigned)ceil_div(c, cc));
    if (store)
        hipLaunchKernelGGL(bev_dense_store_kernel<T>, grid, dim3(256), lds, as_stream(s), (const T *)a, n_rows, c, seg, order, z, cc, hw, (T *)o);
    else
        hipLaunchKernelGGL(bev_dense_gather_kernel<T>, grid, dim3(256), lds, as_stream(s), (const T *)a, n_rows, c, seg, order, z, cc, hw, (T *)o);
    return check_launch(store ? "u2mkd_bev_dense_store" : "u2mkd_bev_dense_gather");
}

static int bev_dense(const char *who, bool store, const void *a, int32_t row_dtype, int64_t n_rows, int32_t c, const int32_t *seg,
                     const int32_t *order, int64_t nb, int32_t z, int32_t h, int32_t w, void *o, u2mkd_stream_t s) {
    U2_REQUIRE(row_dtype >= 0 && row_dtype <= 2, "%s: row dtype %d (0 = fp32, 1 = bf16, 2 = fp16)", who, row_dtype);
    U2_REQUIRE(n_rows >= 0 && nb >= 0 && nb < 65536, "%s: n_rows=%lld, nb=%lld (0 <= nb < 65536)", who, (long long)n_rows, (long long)nb);
    U2_REQUIRE(h > 0 && w > 0 && z > 0, "%s: non-positive shape (z=%d, h=%d, w=%d)", who, z, h, w);
    U2_REQUIRE(z <= 32, "%s: z=%d heights, at most 32", who, z);
    U2_REQUIRE(c > 0 && c % 4 == 0, "%s: c=%d must be a multiple of 4", who, c);
    U2_REQUIRE((seg == nullptr) == (order == nullptr), "%s: seg and order go together", who);
    U2_REQUIRE(seg || (z == 1 && n_rows == nb * (int64_t)h * w), "%s: without seg the rows are the cells (z = 1, n_rows = nb * h * w)", who);
    if (nb == 0) return 0;
    U2_REQUIRE(o && (a || n_rows == 0), "%s: null pointer", who);
    U2_REQUIRE(((uintptr_t)a | (uintptr_t)o) % 16 == 0, "%s: rows and the dense tensor must be 16-byte aligned", who);
    const int64_t hw = (int64_t)h * w;
    if (row_dtype == 0) return bev_dense_launch<float>(store, a, n_rows, c, seg, order, nb, z, hw, o, s);
    if (row_dtype == 1) return bev_dense_launch<bf16row>(store, a, n_rows, c, seg, order, nb, z, hw, o, s);
    return bev_dense_launch<_Float16>(store, a, n_rows, c, seg, order, nb, z, hw, o, s);
}

}  // namespace u2mkd

using namespace u2mkd;

extern "C" {

int u2mkd_bev_plan(const int32_t *coords, int64_t n, int32_t dim, int32_t mode, int32_t hmode, int32_t s0, int32_t s1, int32_t s2,
                   int32_t a0, int32_t a1, int32_t a2, int32_t h, int32_t w, int32_t nz, int64_t *keys, int32_t *hidx,
                   int32_t *block, u2mkd_stream_t s) {
    U2_REQUIRE(dim >= 0 && dim <= 2, "u2mkd_bev_plan: dim=%d outside 0..2", dim);
    U2_REQUIRE(mode == 0 || mode == 1, "u2mkd_bev_plan: mode %d (0 = packed keys, 1 = dense cells)", mode);
    U2_REQUIRE(hmode >= 0 && hmode <= 2 && (hmode != 2 || mode == 1), "u2mkd_bev_plan: hmode %d", hmode);
    U2_REQUIRE(s0 > 0 && s1 > 0 && s2 > 0, "u2mkd_bev_plan: non-positive tensor stride (%d, %d, %d)", s0, s1, s2);
    U2_REQUIRE(mode == 1 || (a0 > 0 && a1 > 0 && a2 > 0), "u2mkd_bev_plan: non-positive cell size (%d, %d, %d)", a0, a1, a2);
    U2_REQUIRE(mode == 0 || (h > 0 && w > 0), "u2mkd_bev_plan: non-positive shape (h=%d, w=%d)", h, w);
    U2_REQUIRE(hmode == 0 || nz > 0, "u2mkd_bev_plan: non-positive shape (heights=%d)", nz);
    U2_REQUIRE(n >= 0, "u2mkd_bev_plan: n=%lld", (long long)n);
    U2_REQUIRE(block && (n == 0 || (coords && keys && hidx)), "u2mkd_bev_plan: null pointer");
    U2_REQUIRE((uintptr_t)coords % 16 == 0, "u2mkd_bev_plan: coords must be 16-byte aligned");
    if (hipMemsetAsync(block, 0, 4 * sizeof(int32_t), as_stream(s)) != hipSuccess) return check_launch("u2mkd_bev_plan") | 1;
    if (n == 0) return 0;
    BevGeom g;
    g.dim = dim;
    g.b0 = dim == 0 ? 1 : 0;
    g.b1 = dim == 2 ? 1 : 2;
    g.mode = mode;
    g.hmode = hmode;
    g.s[0] = s0; g.s[1] = s1; g.s[2] = s2;
    g.a[0] = a0; g.a[1] = a1; g.a[2] = a2;
    g.h = h; g.w = w; g.nz = nz;
    hipLaunchKernelGGL(bev_plan_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(s),
                       reinterpret_cast<const int4 *>(coords), n, g, keys, hidx, block);
    return check_launch("u2mkd_bev_plan");
}

int u2mkd_bev_tables(const int32_t *group, const int32_t *hidx, int64_t n_in, int64_t n_out, int32_t nk, int32_t *nbr,
                     int32_t *nbr_inv, u2mkd_stream_t s) {
    U2_REQUIRE(nk > 0 && n_in >= 0 && n_out >= 0, "u2mkd_bev_tables: non-positive shape (nk=%d, n_in=%lld, n_out=%lld)", nk,
               (long long)n_in, (long long)n_out);
    U2_REQUIRE((n_in == 0 || (group && hidx && nbr_inv)) && (n_out == 0 || nbr), "u2mkd_bev_tables: null pointer");
    const int64_t total = (int64_t)nk * max(n_in, n_out);
    if (total == 0) return 0;
    hipLaunchKernelGGL(bev_tables_fill_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, as_stream(s), group, hidx, n_in,
                       n_out, nk, nbr, nbr_inv);
    if (n_in && n_out)
        hipLaunchKernelGGL(bev_tables_rows_kernel, dim3((unsigned)ceil_div(n_in, 256)), dim3(256), 0, as_stream(s), group, hidx, n_in,
                           n_out, nk, nbr);
    return check_launch("u2mkd_bev_tables");
}

int u2mkd_bev_segment_mean(const void *src, int32_t row_dtype, int64_t n_src, int32_t c, const int32_t *order, const int32_t *seg,
                           int64_t nv, void *out, u2mkd_stream_t s) {
    U2_REQUIRE(row_dtype >= 0 && row_dtype <= 2, "u2mkd_bev_segment_mean: row dtype %d (0 = fp32, 1 = bf16, 2 = fp16)", row_dtype);
    U2_REQUIRE(c > 0 && c % 4 == 0, "u2mkd_bev_segment_mean: c=%d must be a multiple of 4", c);
    U2_REQUIRE(nv >= 0 && n_src >= 0, "u2mkd_bev_segment_mean: nv=%lld, n_src=%lld", (long long)nv, (long long)n_src);
    if (nv == 0) return 0;
    U2_REQUIRE(seg && out && (n_src == 0 || (src && order)), "u2mkd_bev_segment_mean: null pointer");
    U2_REQUIRE(((uintptr_t)src | (uintptr_t)out) % 16 == 0, "u2mkd_bev_segment_mean: rows must be 16-byte aligned");
    const int c4 = c / 4;
    const dim3 grid((unsigned)ceil_div(nv * c4, 256));
    if (row_dtype == 0)
        hipLaunchKernelGGL(bev_segment_mean_kernel<float>, grid, dim3(256), 0, as_stream(s), (const float *)src, c4, n_src, order, seg, nv, (float *)out);
    else if (row_dtype == 1)
        hipLaunchKernelGGL(bev_segment_mean_kernel<bf16row>, grid, dim3(256), 0, as_stream(s), (const bf16row *)src, c4, n_src, order, seg, nv, (bf16row *)out);
    else
        hipLaunchKernelGGL(bev_segment_mean_kernel<_Float16>, grid, dim3(256), 0, as_stream(s), (const _Float16 *)src, c4, n_src, order, seg, nv, (_Float16 *)out);
    return check_launch("u2mkd_bev_segment_mean");
}

int u2mkd_bev_dense_store(const void *src, int32_t row_dtype, int64_t n_rows, int32_t c, const int32_t *seg, const int32_t *order,
                          int64_t nb, int32_t z, int32_t h, int32_t w, void *out, u2mkd_stream_t s) {
    return bev_dense("u2mkd_bev_dense_store", true, src, row_dtype, n_rows, c, seg, order, nb, z, h, w, out, s);
}

int u2mkd_bev_dense_gather(const void *dout, int32_t row_dtype, int64_t n_rows, int32_t c, const int32_t *seg, const int32_t *order,
                           int64_t nb, int32_t z, int32_t h, int32_t w, void *dsrc, u2mkd_stream_t s) {
    return bev_dense("u2mkd_bev_dense_gather", false, dout, row_dtype, n_rows, c, seg, order, nb, z, h, w, dsrc, s);
}

}  // extern "C"
