// Test-time voting tail (u2mkd_amd/evaluate.py: vote_point_predictions): the per-point logits of the V augmented copies of a
// scan, gathered through each copy's inverse map, summed in vote order in fp32, arg-maxed, and counted for MeanIoU -- one
// launch, every size and offset read on the device.
#include "common.h"

namespace u2mkd {
namespace {

constexpr int kVoteThreads = 128;
constexpr int kVoteBlocks = 2048;      // a fixed grid: the point count lives on the device, the points are taken grid-stride
constexpr int kVoteMaxClasses = 64;
constexpr int kVoteMaxCopies = 64;     // device_prep.MAX_BATCH

template <typename T> __device__ __forceinline__ float vote_widen(const T *p, int k);
template <> __device__ __forceinline__ float vote_widen<float>(const float *p, int k) { return p[k]; }
template <> __device__ __forceinline__ float vote_widen<bf16row>(const bf16row *p, int k) {
    return __uint_as_float((uint32_t)p[k].v << 16);      // a bf16 is the upper half of the fp32 with the same value
}
template <> __device__ __forceinline__ float vote_widen<_Float16>(const _Float16 *p, int k) { return (float)p[k]; }

// One thread per output point; its c partial sums stay in registers (CP = c rounded up to an instantiated size) across the
// votes.  Neighbouring threads are neighbouring points of a copy, whose voxel rows are mostly neighbouring or equal.
template <typename T, int CP>
__global__ __launch_bounds__(kVoteThreads) void vote_points_kernel(
    const T *__restrict__ logits, int c, const int64_t *__restrict__ inverse_map, const int32_t *__restrict__ copy_point_off,
    const int32_t *__restrict__ copy_voxel_off, const int32_t *__restrict__ scan_seg, int n_scans, int n_votes,
    const int64_t *__restrict__ targets, int64_t ignore_label, int skip_class, float *__restrict__ sums, int64_t *__restrict__ pred,
    unsigned long long *__restrict__ counts) {
    __shared__ int32_t seg[kVoteMaxCopies + 1];
    __shared__ int32_t point_off[kVoteMaxCopies], voxel_off[kVoteMaxCopies];      // the copies' tables: read once per workgroup
    __shared__ uint32_t hist[3 * kVoteMaxClasses];      // seen, correct, predicted
    const int tid = threadIdx.x;
    for (int i = tid; i <= n_scans; i += kVoteThreads) seg[i] = scan_seg[i];
    for (int i = tid; i < n_scans * n_votes; i += kVoteThreads) {
        point_off[i] = copy_point_off[i];
        voxel_off[i] = copy_voxel_off[i];
    }
    for (int i = tid; i < 3 * kVoteMaxClasses; i += kVoteThreads) hist[i] = 0u;
    __syncthreads();
    const int64_t n_points = seg[n_scans];
    for (int64_t p = (int64_t)blockIdx.x * kVoteThreads + tid; p < n_points; p += (int64_t)gridDim.x * kVoteThreads) {
        int lo = 0, hi = n_scans;                      // seg[lo] <= p < seg[hi]; empty scans own no point
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)seg[mid] <= p) lo = mid; else hi = mid;
        }
        const int64_t j = p - seg[lo];
        float acc[CP];
#pragma unroll
        for (int k = 0; k < CP; ++k) acc[k] = 0.f;
        for (int v = 0; v < n_votes; ++v) {
            const int b = lo * n_votes + v;
            const int64_t row = (int64_t)voxel_off[b] + inverse_map[(int64_t)point_off[b] + j];
            const T *r = logits + row * c;
#pragma unroll
            for (int k = 0; k < CP; ++k)
                if (k < c) acc[k] += vote_widen<T>(r, k);
        }
        // the lowest index among the maxima; a NaN is maximal (the first one wins), as torch.argmax on the CPU and numpy
        int best = -1;
        float best_v = 0.f;
#pragma unroll
        for (int k = 0; k < CP; ++k) {
            if (k < c && k != skip_class) {
                const float x = acc[k];
                if (best < 0 || x > best_v || (x != x && best_v == best_v)) {
                    best = k;
                    best_v = x;
                }
            }
        }
        pred[p] = best;
        if (sums) {
            float *o = sums + p * c;
#pragma unroll
            for (int k = 0; k < CP; ++k)
                if (k < c) o[k] = acc[k];
        }
        if (counts) {
            const int64_t t = targets[p];
            if (t != ignore_label && t >= 0 && t < c) {
                atomicAdd(&hist[(int)t], 1u);
                if (best == (int)t) atomicAdd(&hist[kVoteMaxClasses + (int)t], 1u);
                atomicAdd(&hist[2 * kVoteMaxClasses + best], 1u);
            }
        }
    }
    if (counts) {      // (uniform: a kernel argument)
        __syncthreads();
        for (int i = tid; i < 3 * kVoteMaxClasses; i += kVoteThreads) {
            const int k = i % kVoteMaxClasses;
            if (k < c && hist[i]) atomicAdd(counts + (i / kVoteMaxClasses) * c + k, (unsigned long long)hist[i]);
        }
    }
}

template <typename T>
void vote_launch(const void *logits, int32_t c, const int64_t *inverse_map, const int32_t *copy_point_off,
                 const int32_t *copy_voxel_off, const int32_t *scan_seg, int32_t n_scans, int32_t n_votes, const int64_t *targets,
                 int64_t ignore_label, int32_t skip_class, float *sums, int64_t *pred, int64_t *counts, hipStream_t st) {
    const T *x = reinterpret_cast<const T *>(logits);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts);
#define U2_VOTE_LAUNCH(CP)                                                                                                        \
    hipLaunchKernelGGL((vote_points_kernel<T, CP>), dim3(kVoteBlocks), dim3(kVoteThreads), 0, st, x, c, inverse_map, copy_point_off, \
                       copy_voxel_off, scan_seg, n_scans, n_votes, targets, ignore_label, skip_class, sums, pred, cnt)
    if (c <= 8) U2_VOTE_LAUNCH(8);
    else if (c <= 24) U2_VOTE_LAUNCH(24);
    else U2_VOTE_LAUNCH(64);
#undef U2_VOTE_LAUNCH
}

}  // namespace
}  // namespace u2mkd

using namespace u2mkd;

extern "C" {

int u2mkd_vote_points(const void *logits, int32_t row_type, int32_t c, const int64_t *inverse_map, const int32_t *copy_point_off,
                      const int32_t *copy_voxel_off, const int32_t *scan_seg, int32_t n_scans, int32_t n_votes,
                      const int64_t *targets, int64_t ignore_label, int32_t skip_class, float *sums, int64_t *pred, int64_t *counts,
                      u2mkd_stream_t s) {
    U2_REQUIRE(row_type >= 0 && row_type <= 2, "u2mkd_vote_points: row_type %d (0 = fp32, 1 = bf16, 2 = fp16)", row_type);
    U2_REQUIRE(c >= 1 && c <= kVoteMaxClasses, "u2mkd_vote_points: 1 <= c <= %d, got %d", kVoteMaxClasses, c);
    U2_REQUIRE(n_votes >= 1, "u2mkd_vote_points: n_votes >= 1, got %d", n_votes);
    U2_REQUIRE(n_scans >= 0, "u2mkd_vote_points: n_scans >= 0, got %d", n_scans);
    U2_REQUIRE((int64_t)n_scans * n_votes <= kVoteMaxCopies, "u2mkd_vote_points: n_scans * n_votes <= %d, got %d * %d", kVoteMaxCopies,
               n_scans, n_votes);
    U2_REQUIRE(skip_class < c, "u2mkd_vote_points: skip_class %d is not a class of %d", skip_class, c);
    U2_REQUIRE(skip_class < 0 || c >= 2, "u2mkd_vote_points: skip_class leaves no class to predict (c = 1)");
    if (n_scans == 0) return 0;
    U2_REQUIRE(logits && inverse_map && copy_point_off && copy_voxel_off && scan_seg && pred, "u2mkd_vote_points: NULL argument");
    U2_REQUIRE(!counts || targets, "u2mkd_vote_points: counts without targets");
    hipStream_t st = as_stream(s);
    if (row_type == 0)
        vote_launch<float>(logits, c, inverse_map, copy_point_off, copy_voxel_off, scan_seg, n_scans, n_votes, targets, ignore_label,
                           skip_class, sums, pred, counts, st);
    else if (row_type == 1)
        vote_launch<bf16row>(logits, c, inverse_map, copy_point_off, copy_voxel_off, scan_seg, n_scans, n_votes, targets, ignore_label,
                             skip_class, sums, pred, counts, st);
    else
        vote_launch<_Float16>(logits, c, inverse_map, copy_point_off, copy_voxel_off, scan_seg, n_scans, n_votes, targets,
                              ignore_label, skip_class, sums, pred, counts, st);
    return check_launch("u2mkd_vote_points");
}

}  // extern "C"
