// Loader geometry on the device (u2mkd_amd/data/device_prep.py): what data/nuscenes_lc.py computes per sample in numpy --
// multi-sweep aggregation, rotate / scale / flip, voxelisation, the LiDAR -> camera projection chain, first-point voxel sets
// (sparse_quantize) and the gathers by `inds` -- for a whole batch, from the raw arrays a loader worker read.
//
// ARITHMETIC RULE.  Every floating-point operation below is one IEEE multiply, add or divide with one rounding, in the
// written order, NEVER contracted into a fused multiply-add: the results are compared bit for bit with numpy's elementwise
// kernels (tests/device_prep_ref.py).  The file is compiled with -ffp-contract=off (build.py) and repeats it here for any
// other build; float32 division is the correctly rounded one (hipcc's default).  No float atomics: the only atomics are
// integer minima and a flag, both order-independent.
#include "common.h"

#pragma clang fp contract(off)

namespace u2mkd {

constexpr int kPrepThreads = 256;          // 4 waves
constexpr int kPrepScanBlock = 2048;       // elements per scan workgroup (256 threads x 8)
constexpr int64_t kPrepPadKey = 0x7fffffffffffffffLL;      // key of the slots behind the last point: sorts last
constexpr int kKeyBitsX = 20, kKeyBitsY = 20, kKeyBitsZ = 16;      // + 7 bits of sample index: 63 bits, never the pad key

// largest b in [0, count) with seg[b] <= i (seg[0] = 0 <= i): the segment that holds i, empty segments skipped
__device__ __forceinline__ int seg_find(const int32_t *__restrict__ seg, int count, int64_t i) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- exclusive prefix sum of int32 flags: out[i] = flags[0] + ... + flags[i-1], out[n] = the total -----------------------
__global__ void __launch_bounds__(kPrepThreads)
prep_block_sums_kernel(const int32_t *__restrict__ flags, int64_t n, int32_t *__restrict__ block_sums) {
    __shared__ int s[kPrepThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kPrepScanBlock;
    int t = 0;
#pragma unroll
    for (int j = 0; j < kPrepScanBlock / kPrepThreads; ++j) {
        const int64_t i = base + threadIdx.x + j * kPrepThreads;
        t += i < n ? flags[i] : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_down(t, off);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ void __launch_bounds__(kPrepThreads)
prep_scan_blocks_kernel(const int32_t *__restrict__ flags, int64_t n, const int32_t *__restrict__ block_sums, int nb,
                        int32_t *__restrict__ out /*[n+1]*/) {
    __shared__ int s_pre[kPrepThreads / 64], s_tot[kPrepThreads / 64], s[kPrepThreads / 64];
    int pre = 0, tot = 0;
    for (int b = threadIdx.x; b < nb; b += kPrepThreads) {
        const int v = block_sums[b];
        tot += v;
        pre += b < (int)blockIdx.x ? v : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pre += __shfl_down(pre, off);
        tot += __shfl_down(tot, off);
    }
    if ((threadIdx.x & 63) == 0) { s_pre[threadIdx.x >> 6] = pre; s_tot[threadIdx.x >> 6] = tot; }
    __syncthreads();
    const int block_off = s_pre[0] + s_pre[1] + s_pre[2] + s_pre[3];
    const int64_t base = (int64_t)blockIdx.x * kPrepScanBlock + (int64_t)threadIdx.x * 8;
    int v[8], sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = base + j < n ? flags[base + j] : 0;
        sum += v[j];
    }
    int incl = sum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s[wave] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += s[w];
    int run = block_off + woff + incl - sum;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
}

// ---- sweeps: the 1 m close-point filter (_aggregate_lidar_sweeps: |x| < 1 and |y| < 1 are dropped) ------------------------
__global__ void __launch_bounds__(kPrepThreads)
prep_sweep_keep_kernel(const float4 *__restrict__ sweep, int64_t m, int32_t *__restrict__ keep) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const float4 p = sweep[j];
    keep[j] = (fabsf(p.x) < 1.0f && fabsf(p.y) < 1.0f) ? 0 : 1;      // (a NaN coordinate is not "close": kept, as numpy keeps it)
}

// ---- points of one network input: aggregate, augment, voxelise -----------------------------------------------------------
// Thread i < nk: key-frame point i; thread nk + j: sweep point j (only where keep[j]).  Sample b's points land behind each
// other -- its key-frame points, then its kept sweep points in sweep order and original order (pos = the exclusive scan of
// keep over ALL sweep points of the batch, so the placement is stable):
//     key-frame point i  -> i + pos[mseg[b]]            sweep point j -> kseg[b + 1] + pos[j]
// par[b] = rot[9] (row-major), scale.  train = 0: nothing is rotated.  f32mode: the loader's points are float32 (no sweeps:
// `out = np.zeros_like(pts)`; the student always), so the double products are rounded to float32 BEFORE the voxel division,
// which is then a float32 division by (float)voxel_size; otherwise everything stays double.
__global__ void __launch_bounds__(kPrepThreads)
prep_points_kernel(const float4 *__restrict__ key, const int64_t *__restrict__ labels, int64_t nk,
                   const float4 *__restrict__ sweep, int64_t m, const int32_t *__restrict__ keep, const int32_t *__restrict__ pos,
                   const int32_t *__restrict__ kseg, const int32_t *__restrict__ mseg, const int32_t *__restrict__ sseg,
                   int32_t n_sweeps, const double *__restrict__ tm, int32_t nb, const double *__restrict__ par,
                   const int32_t *__restrict__ flip, int32_t train, int32_t f32mode, double voxel_size, int64_t ignore_label,
                   float4 *__restrict__ feats, int4 *__restrict__ vox, int64_t *__restrict__ labels_full,
                   uint8_t *__restrict__ kf, int32_t *__restrict__ mn, int32_t *__restrict__ off) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= nb) off[i] = kseg[i] + pos[mseg[i]];
    if (i >= nk + m) return;
    int b;
    int64_t dest;
    double x, y, z;
    float w;
    int64_t label;
    bool is_key;
    if (i < nk) {
        b = seg_find(kseg, nb, i);
        dest = i + pos[mseg[b]];
        const float4 p = key[i];
        x = (double)p.x; y = (double)p.y; z = (double)p.z; w = p.w;
        label = labels ? labels[i] : 0;
        is_key = true;
    } else {
        const int64_t j = i - nk;
        if (!keep[j]) return;
        b = seg_find(mseg, nb, j);
        dest = (int64_t)kseg[b + 1] + pos[j];
        const double *t = tm + (int64_t)seg_find(sseg, n_sweeps, j) * 16;
        const float4 p = sweep[j];
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        x = ((px * t[0] + py * t[1]) + pz * t[2]) + t[3];
        y = ((px * t[4] + py * t[5]) + pz * t[6]) + t[7];
        z = ((px * t[8] + py * t[9]) + pz * t[10]) + t[11];
        w = p.w;
        label = ignore_label;
        is_key = false;        // `lag` is never 0 for a real sweep: the loader's `agg_ts == 0` is "is a key-frame point"
    }
    if (train) {
        const double *r = par + (int64_t)b * 10;
        const double scale = r[9];
        const double ox = ((x * r[0] + y * r[3]) + z * r[6]) * scale;
        const double oy = ((x * r[1] + y * r[4]) + z * r[7]) * scale;
        const double oz = ((x * r[2] + y * r[5]) + z * r[8]) * scale;
        x = ox; y = oy; z = oz;
        const int kind = flip[b];
        if (kind == 1 || kind == 3) x = -x;
        if (kind == 2 || kind == 3) y = -y;
    }
    int vx, vy, vz;
    float4 f;
    f.x = (float)x; f.y = (float)y; f.z = (float)z; f.w = w;
    if (f32mode) {
        const float vs = (float)voxel_size;
        vx = (int)rintf(f.x / vs); vy = (int)rintf(f.y / vs); vz = (int)rintf(f.z / vs);
    } else {
        vx = (int)rint(x / voxel_size); vy = (int)rint(y / voxel_size); vz = (int)rint(z / voxel_size);
    }
    feats[dest] = f;
    vox[dest] = make_int4(vx, vy, vz, b);
    if (labels_full) labels_full[dest] = label;
    if (kf) kf[dest] = is_key ? 1 : 0;
    atomicMin(&mn[3 * b + 0], vx);          // (an integer minimum does not depend on the order)
    atomicMin(&mn[3 * b + 1], vy);
    atomicMin(&mn[3 * b + 2], vz);
}

// ---- LiDAR -> camera projection of the key-frame points -------------------------------------------------------------------
// cam[(b * ncam + c) * 60]: four (R[9], t[3]) steps -- lidar -> ego, ego -> global (p = R p + t), global -> ego at camera time,
// ego -> camera (p = R^T (p - t)) -- then K[9], im_w - 1, im_h - 1, pad.
constexpr int kCamStride = 60;
__global__ void __launch_bounds__(kPrepThreads)
prep_project_kernel(const float4 *__restrict__ key, int64_t nk, const int32_t *__restrict__ kseg, int32_t nb, int32_t ncam,
                    const double *__restrict__ cam, float2 *__restrict__ pc /*[ncam, nk]*/, uint8_t *__restrict__ masks /*[ncam, nk]*/,
                    uint8_t *__restrict__ pt_with_img /*[nk]*/) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nk) return;
    const int b = seg_find(kseg, nb, i);
    const float4 p4 = key[i];
    bool any = false;
    for (int c = 0; c < ncam; ++c) {
        const double *q = cam + ((int64_t)b * ncam + c) * kCamStride;
        double x = (double)p4.x, y = (double)p4.y, z = (double)p4.z;
#pragma unroll
        for (int step = 0; step < 2; ++step, q += 12) {
            const double nx = ((q[0] * x + q[1] * y) + q[2] * z) + q[9];
            const double ny = ((q[3] * x + q[4] * y) + q[5] * z) + q[10];
            const double nz = ((q[6] * x + q[7] * y) + q[8] * z) + q[11];
            x = nx; y = ny; z = nz;
        }
#pragma unroll
        for (int step = 0; step < 2; ++step, q += 12) {
            const double dx = x - q[9], dy = y - q[10], dz = z - q[11];
            x = (q[0] * dx + q[3] * dy) + q[6] * dz;
            y = (q[1] * dx + q[4] * dy) + q[7] * dz;
            z = (q[2] * dx + q[5] * dy) + q[8] * dz;
        }
        const bool front = z > 1.0;
        const double kx = (q[0] * x + q[1] * y) + q[2] * z;
        const double ky = (q[3] * x + q[4] * y) + q[5] * z;
        const double kz = (q[6] * x + q[7] * y) + q[8] * z;
        const double u = (kx / kz) / q[9] * 2.0 - 1.0;
        const double v = (ky / kz) / q[10] * 2.0 - 1.0;
        const bool in = front && u > -1.0 && u < 1.0 && v > -1.0 && v < 1.0;      // strict; a NaN fails every comparison
        pc[(int64_t)c * nk + i] = make_float2((float)u, (float)v);
        masks[(int64_t)c * nk + i] = in ? 1 : 0;
        any = any || in;
    }
    pt_with_img[i] = any ? 1 : 0;
}

// ---- first-point voxel sets (sparse_quantize) ----------------------------------------------------------------------------
// key = (sample, x, y, z) of the min-subtracted voxel, packed lexicographically: the order of ravel_hash within a sample.
__global__ void __launch_bounds__(kPrepThreads)
prep_voxel_keys_kernel(const int4 *__restrict__ vox, const int32_t *__restrict__ mn, const int32_t *__restrict__ off, int32_t nb,
                       int64_t cap, int64_t *__restrict__ keys, int32_t *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    if (i >= off[nb]) { keys[i] = kPrepPadKey; return; }
    const int4 v = vox[i];
    const int64_t x = (int64_t)v.x - mn[3 * v.w], y = (int64_t)v.y - mn[3 * v.w + 1], z = (int64_t)v.z - mn[3 * v.w + 2];
    const bool fits = x >= 0 && x < (1LL << kKeyBitsX) && y >= 0 && y < (1LL << kKeyBitsY) && z >= 0 && z < (1LL << kKeyBitsZ);
    if (!fits) atomicOr(err, 1);
    const int64_t cx = fits ? x : 0, cy = fits ? y : 0, cz = fits ? z : 0;
    keys[i] = ((((int64_t)v.w << kKeyBitsX | cx) << kKeyBitsY | cy) << kKeyBitsZ) | cz;
}

__global__ void __launch_bounds__(kPrepThreads)
prep_heads_kernel(const int64_t *__restrict__ skeys, int64_t cap, int32_t *__restrict__ head) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cap) return;
    const int64_t k = skeys[j];
    head[j] = (k != kPrepPadKey && (j == 0 || skeys[j - 1] != k)) ? 1 : 0;
}

// sorted slot j (a STABLE sort: the first slot of a run of equal keys holds the smallest point index): the point's voxel rank,
// and for the head of a voxel the gather of every per-point array by `inds`, the batch index appended to the coordinates.
// The per-camera arrays of sample b are laid out [ncam, nv_b] behind those of the samples before it.
__global__ void __launch_bounds__(kPrepThreads)
prep_finish_kernel(const int64_t *__restrict__ skeys, const int64_t *__restrict__ perm, const int32_t *__restrict__ head,
                   const int32_t *__restrict__ rank /*[cap+1]*/, int64_t cap, const int32_t *__restrict__ off, int32_t nb,
                   const float4 *__restrict__ feats, const int4 *__restrict__ vox, const int32_t *__restrict__ mn,
                   const int64_t *__restrict__ labels, const uint8_t *__restrict__ kf, const uint8_t *__restrict__ pt_with_img,
                   const uint8_t *__restrict__ masks, const float2 *__restrict__ pc, int32_t ncam, int64_t nk,
                   int64_t *__restrict__ inverse_map, int64_t *__restrict__ inds, float4 *__restrict__ feats_o,
                   int4 *__restrict__ coords_o, int64_t *__restrict__ labels_o, uint8_t *__restrict__ kf_o,
                   uint8_t *__restrict__ fov_o, uint8_t *__restrict__ masks_o, float2 *__restrict__ pc_o,
                   int32_t *__restrict__ voxoff /*[nb+1]*/) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= nb) voxoff[j] = rank[off[j]];
    if (j >= cap) return;
    const int64_t k = skeys[j];
    if (k == kPrepPadKey) return;
    const int b = (int)(k >> (kKeyBitsX + kKeyBitsY + kKeyBitsZ));
    const int64_t p = perm[j];
    const int h = head[j];
    const int64_t v = (int64_t)rank[j] + h - 1;
    const int64_t v0 = rank[off[b]];
    inverse_map[p] = v - v0;
    if (!h) return;
    inds[v] = p - off[b];
    feats_o[v] = feats[p];
    const int4 c = vox[p];
    coords_o[v] = make_int4(c.x - mn[3 * b], c.y - mn[3 * b + 1], c.z - mn[3 * b + 2], b);
    labels_o[v] = labels[p];
    if (kf_o) kf_o[v] = kf[p];
    if (fov_o) fov_o[v] = pt_with_img[p];
    if (masks_o) {
        const int64_t nv = (int64_t)rank[off[b + 1]] - v0;
        for (int cm = 0; cm < ncam; ++cm) {
            const int64_t o = (int64_t)ncam * v0 + (int64_t)cm * nv + (v - v0);
            masks_o[o] = masks[(int64_t)cm * nk + p];
            pc_o[o] = pc[(int64_t)cm * nk + p];
        }
    }
}

static int prep_scan(const int32_t *flags, int64_t n, int32_t *out, int32_t *block_sums, hipStream_t st) {
    if (n == 0) {
        (void)hipMemsetAsync(out, 0, sizeof(int32_t), st);
        return 0;
    }
    const int nb = (int)ceil_div(n, kPrepScanBlock);
    hipLaunchKernelGGL(prep_block_sums_kernel, dim3(nb), dim3(kPrepThreads), 0, st, flags, n, block_sums);
    hipLaunchKernelGGL(prep_scan_blocks_kernel, dim3(nb), dim3(kPrepThreads), 0, st, flags, n, block_sums, nb, out);
    return 0;
}

}  // namespace u2mkd

using namespace u2mkd;

extern "C" {

size_t u2mkd_prep_scan_workspace_bytes(int64_t n) {
    return (size_t)(n + ceil_div(n > 0 ? n : 1, kPrepScanBlock)) * sizeof(int32_t);
}

int32_t u2mkd_prep_key_bits(int32_t axis) {
    return axis == 0 ? kKeyBitsX : axis == 1 ? kKeyBitsY : axis == 2 ? kKeyBitsZ : 63 - kKeyBitsX - kKeyBitsY - kKeyBitsZ;
}

int u2mkd_prep_sweep_compact(const float *sweep, int64_t m, void *workspace, int32_t *pos, u2mkd_stream_t s) {
    U2_REQUIRE(m >= 0 && m < ((int64_t)1 << 31) - kPrepScanBlock, "u2mkd_prep_sweep_compact: size out of range");
    U2_REQUIRE(pos && (m == 0 || (sweep && workspace)), "u2mkd_prep_sweep_compact: null pointer");
    hipStream_t st = as_stream(s);
    int32_t *keep = reinterpret_cast<int32_t *>(workspace);
    if (m)
        hipLaunchKernelGGL(prep_sweep_keep_kernel, dim3((unsigned)ceil_div(m, kPrepThreads)), dim3(kPrepThreads), 0, st,
                           reinterpret_cast<const float4 *>(sweep), m, keep);
    prep_scan(keep, m, pos, keep + m, st);
    return check_launch("u2mkd_prep_sweep_compact");
}

int u2mkd_prep_points(const float *key, const int64_t *labels, int64_t nk, const float *sweep, int64_t m, const void *workspace,
                      const int32_t *pos, const int32_t *kseg, const int32_t *mseg, const int32_t *sseg, int32_t n_sweeps,
                      const double *tm, int32_t nb, const double *par, const int32_t *flip, int32_t train, int32_t f32mode,
                      double voxel_size, int64_t ignore_label, float *feats, int32_t *vox, int64_t *labels_full, uint8_t *kf,
                      int32_t *mn, int32_t *off, u2mkd_stream_t s) {
    U2_REQUIRE(nk >= 0 && m >= 0 && nk + m < ((int64_t)1 << 31) - kPrepScanBlock, "u2mkd_prep_points: size out of range");
    U2_REQUIRE(nb >= 1 && nb <= 64, "u2mkd_prep_points: 1 to 64 samples per batch");
    U2_REQUIRE(pos && kseg && mseg && mn && off && (nk + m == 0 || (feats && vox)) && (nk == 0 || key), "u2mkd_prep_points: null pointer");
    U2_REQUIRE(m == 0 || (sweep && workspace && sseg && tm && n_sweeps >= 1), "u2mkd_prep_points: sweep points without their tables");
    U2_REQUIRE(!train || (par && flip), "u2mkd_prep_points: training mode without augmentation parameters");
    U2_REQUIRE(voxel_size > 0, "u2mkd_prep_points: voxel_size must be positive");
    const int64_t threads = nk + m > nb + 1 ? nk + m : nb + 1;
    hipLaunchKernelGGL(prep_points_kernel, dim3((unsigned)ceil_div(threads, kPrepThreads)), dim3(kPrepThreads), 0, as_stream(s),
                       reinterpret_cast<const float4 *>(key), labels, nk, reinterpret_cast<const float4 *>(sweep), m,
                       reinterpret_cast<const int32_t *>(workspace), pos, kseg, mseg, sseg, n_sweeps, tm, nb, par, flip, train,
                       f32mode, voxel_size, ignore_label, reinterpret_cast<float4 *>(feats), reinterpret_cast<int4 *>(vox),
                       labels_full, kf, mn, off);
    return check_launch("u2mkd_prep_points");
}

int u2mkd_prep_project(const float *key, int64_t nk, const int32_t *kseg, int32_t nb, int32_t ncam, const double *cam, float *pc,
                       uint8_t *masks, uint8_t *pt_with_img, u2mkd_stream_t s) {
    U2_REQUIRE(nk >= 0 && nb >= 1 && ncam >= 1 && ncam <= 16, "u2mkd_prep_project: sizes out of range");
    U2_REQUIRE(kseg && cam && (nk == 0 || (key && pc && masks && pt_with_img)), "u2mkd_prep_project: null pointer");
    if (nk)
        hipLaunchKernelGGL(prep_project_kernel, dim3((unsigned)ceil_div(nk, kPrepThreads)), dim3(kPrepThreads), 0, as_stream(s),
                           reinterpret_cast<const float4 *>(key), nk, kseg, nb, ncam, cam, reinterpret_cast<float2 *>(pc), masks,
                           pt_with_img);
    return check_launch("u2mkd_prep_project");
}

int u2mkd_prep_voxel_keys(const int32_t *vox, const int32_t *mn, const int32_t *off, int32_t nb, int64_t cap, int64_t *keys,
                          int32_t *err, u2mkd_stream_t s) {
    U2_REQUIRE(cap >= 0 && nb >= 1 && nb <= 64, "u2mkd_prep_voxel_keys: sizes out of range");
    U2_REQUIRE(mn && off && err && (cap == 0 || (vox && keys)), "u2mkd_prep_voxel_keys: null pointer");
    if (cap)
        hipLaunchKernelGGL(prep_voxel_keys_kernel, dim3((unsigned)ceil_div(cap, kPrepThreads)), dim3(kPrepThreads), 0, as_stream(s),
                           reinterpret_cast<const int4 *>(vox), mn, off, nb, cap, keys, err);
    return check_launch("u2mkd_prep_voxel_keys");
}

int u2mkd_prep_voxel_sets(const int64_t *skeys, const int64_t *perm, int64_t cap, void *workspace, int32_t *rank,
                          const int32_t *off, int32_t nb, const float *feats, const int32_t *vox, const int32_t *mn,
                          const int64_t *labels, const uint8_t *kf, const uint8_t *pt_with_img, const uint8_t *masks,
                          const float *pc, int32_t ncam, int64_t nk, int64_t *inverse_map, int64_t *inds, float *feats_o,
                          int32_t *coords_o, int64_t *labels_o, uint8_t *kf_o, uint8_t *fov_o, uint8_t *masks_o, float *pc_o,
                          int32_t *voxoff, u2mkd_stream_t s) {
    U2_REQUIRE(cap >= 0 && cap < ((int64_t)1 << 31) - kPrepScanBlock && nb >= 1 && nb <= 64, "u2mkd_prep_voxel_sets: sizes out of range");
    U2_REQUIRE(rank && off && mn && voxoff && workspace, "u2mkd_prep_voxel_sets: null pointer");
    U2_REQUIRE(cap == 0 || (skeys && perm && feats && vox && labels && inverse_map && inds && feats_o && coords_o && labels_o),
               "u2mkd_prep_voxel_sets: null pointer");
    U2_REQUIRE(!kf_o || kf, "u2mkd_prep_voxel_sets: keyframe output without its input");
    U2_REQUIRE(!fov_o || pt_with_img, "u2mkd_prep_voxel_sets: fov output without its input");
    U2_REQUIRE(!masks_o || (masks && pc && pc_o && ncam >= 1), "u2mkd_prep_voxel_sets: camera outputs without their inputs");
    hipStream_t st = as_stream(s);
    int32_t *head = reinterpret_cast<int32_t *>(workspace);
    if (cap)
        hipLaunchKernelGGL(prep_heads_kernel, dim3((unsigned)ceil_div(cap, kPrepThreads)), dim3(kPrepThreads), 0, st, skeys, cap, head);
    prep_scan(head, cap, rank, head + cap, st);
    const int64_t threads = cap > nb + 1 ? cap : nb + 1;
    hipLaunchKernelGGL(prep_finish_kernel, dim3((unsigned)ceil_div(threads, kPrepThreads)), dim3(kPrepThreads), 0, st, skeys, perm,
                       head, rank, cap, off, nb, reinterpret_cast<const float4 *>(feats), reinterpret_cast<const int4 *>(vox), mn,
                       labels, kf, pt_with_img, masks, reinterpret_cast<const float2 *>(pc), ncam, nk, inverse_map, inds,
                       reinterpret_cast<float4 *>(feats_o), reinterpret_cast<int4 *>(coords_o), labels_o, kf_o, fov_o, masks_o,
                       reinterpret_cast<float2 *>(pc_o), voxoff);
    return check_launch("u2mkd_prep_voxel_sets");
}

}  // extern "C"
