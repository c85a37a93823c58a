// Sparse 3D convolution with LARGE KERNEL VOLUMES (32 < K <= 343: k = 5, k = 7, 3x3x5, k4s4) on gfx950: the output-stationary
// contraction of conv_os2_kernel (conv.hip) with the offsets walked in CHUNKS OF 32.
//
//   out[j] = sum_k in[nbr[k][j]] * B_k,   B_k = wt[kflip ? K-1-k : k] as [cout][cin]
//
// conv_os2 / conv_os3 and the tile kernels load a tile's [K][TM] neighbour indices in one burst sized for 32 offsets and walk ONE
// 32-bit offset mask; a row-mask sort and a tile schedule (K <= 31) put rows of equal masks together.  Here
//   * a workgroup (4 waves) owns 64 output rows IN NATURAL ORDER and 16 * NB output columns; the accumulators stay in registers
//     from the first offset to the store (one running fp32 sum per element, v_mfma_f32_16x16x4_f32: an exact fp32 fma chain);
//   * per chunk of 32 offsets: one burst of index loads into the LDS image [32][64] (the loads of chunk c + 1 are issued before
//     the products of chunk c), the waves' 32-bit masks are ORed, and only the offsets the tile has are visited -- a chunk
//     without a live offset costs its index burst and one barrier;
//   * per (live offset, KC-channel step): B_k's tile goes through LDS once for the 4 waves, a wave gathers its 16 rows straight
//     into the A operand, the global loads of step s + 1 are issued before the products of step s (conv_os2's pipeline; it is
//     drained at the end of a chunk); a wave whose 16 rows have no neighbour at the offset skips its products by ballot;
//   * kflip mirrors over the WHOLE volume (K - 1 - k);
//   * every element of out is stored exactly once -- a row without any neighbour as exact zeros -- no atomics, no memset, a fixed
//     summation order: the same bits on every run.
// An index outside [0, n_in) counts as "no neighbour" (nothing is gathered through it).
#include "conv_internal.h"

namespace u2mkd {

constexpr int kLkMaxVolume = 343;   // 7 x 7 x 7

template <int NB, int KC>
__global__ void __launch_bounds__(256)
conv_lk_kernel(const float *__restrict__ in, int64_t n_in, int cin, const float *__restrict__ wt, int cout,
               const int32_t *__restrict__ nbr, int64_t ld, int64_t n_rows, int K, int kflip, float *__restrict__ out) {
    constexpr int WAVES = 4, NT = 64 * WAVES, TM = 16 * WAVES, TN = 16 * NB;
    constexpr int BS = KC + 8;                          // LDS row stride (floats): a lane's ds_read_b128 is conflict free
    constexpr int F4ROW = KC / 4;                       // float4 per B row
    constexpr int BPASS = (TN * F4ROW + NT - 1) / NT;   // float4 B loads per thread per step
    constexpr int NJ = KC / 16;
    constexpr int IT = 32 * TM / NT;                    // index loads per thread per chunk
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *Bs = reinterpret_cast<float *>(smem);                       // [2][TN][BS]
    int *s_idx = reinterpret_cast<int *>(Bs + 2 * TN * BS);            // [32][TM]
    unsigned *s_wmask = reinterpret_cast<unsigned *>(s_idx + 32 * TM); // [2][WAVES]: by chunk parity (an empty chunk has no
                                                                       // barrier between its read and the next chunk's write)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int col0 = blockIdx.y * TN;
    const int64_t row0 = (int64_t)blockIdx.x * TM;
    const int nstep = (cin + KC - 1) / KC;
    const int nchunk = (K + 31) / 32;
    const int wrow = 16 * wave;   // first tile-local row of this wave

    f32x4 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int v[IT];
    auto load_indices = [&](int chunk) {   // thread tid holds offsets wave + 4 i of the chunk, row `lane`
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = tid + i * NT;
            const int kg = 32 * chunk + e / TM;
            const int64_t row = row0 + (e % TM);
            v[i] = (kg < K && row < n_rows) ? nbr[(int64_t)kg * ld + row] : -1;
        }
    };
    load_indices(0);

    float4 a_cur[NJ], a_nxt[NJ], breg[BPASS];
    bool act_cur = false, act_nxt = false;

    for (int chunk = 0; chunk < nchunk; ++chunk) {
        const int k0 = 32 * chunk;
        unsigned mymask = 0u;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = tid + i * NT;
            int x = v[i];
            if (x < 0 || (int64_t)x >= n_in) x = -1;
            s_idx[e] = x;
            if (x >= 0) mymask |= 1u << (e / TM);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mymask |= __shfl_xor(mymask, off);
        unsigned *wm = s_wmask + (chunk & 1) * WAVES;
        if (lane == 0) wm[wave] = mymask;
        __syncthreads();
        unsigned km = wm[0] | wm[1] | wm[2] | wm[3];
        if (chunk + 1 < nchunk) load_indices(chunk + 1);
        if (!km) continue;

        auto load_stage = [&](int k, int c, float4 (&a)[NJ], bool &active) {
            const int kg = k0 + k;
            const float *wk = wt + (size_t)((kflip & 1) ? K - 1 - kg : kg) * cout * cin;
#pragma unroll
            for (int p = 0; p < BPASS; ++p) {
                int f = tid + NT * p;
                int col = f / F4ROW, ci = c * KC + (f % F4ROW) * 4;
                breg[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (col < TN && col0 + col < cout && ci < cin)
                    breg[p] = *reinterpret_cast<const float4 *>(wk + (size_t)(col0 + col) * cin + ci);
            }
            int idx = s_idx[k * TM + wrow + r];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                int ci = c * KC + 16 * j + 4 * q;
                a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (idx >= 0 && ci < cin) a[j] = *reinterpret_cast<const float4 *>(in + (size_t)idx * cin + ci);
            }
            active = __ballot(idx >= 0) != 0ULL;
        };
        auto store_B = [&](int buf) {
#pragma unroll
            for (int p = 0; p < BPASS; ++p) {
                int f = tid + NT * p;
                int col = f / F4ROW;
                if (col < TN)
                    *reinterpret_cast<float4 *>(Bs + ((size_t)buf * TN + col) * BS + (f % F4ROW) * 4) = breg[p];
            }
        };

        int k = __builtin_ctz(km);
        km &= km - 1;
        int c = 0;
        load_stage(k, 0, a_cur, act_cur);
        store_B(0);
        __syncthreads();
        int buf = 0;
        while (true) {
            int kn = k, cn = c + 1;
            bool have_next = true;
            if (cn == nstep) {
                cn = 0;
                if (km) { kn = __builtin_ctz(km); km &= km - 1; } else have_next = false;
            }
            if (have_next) load_stage(kn, cn, a_nxt, act_nxt);
            if (act_cur) {
                const float *bb = Bs + (size_t)buf * TN * BS + r * BS + 4 * q;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    float4 b[NB];
#pragma unroll
                    for (int n = 0; n < NB; ++n) b[n] = *reinterpret_cast<const float4 *>(bb + 16 * n * BS + 16 * j);
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[j].x, b[n].x, acc[n], 0, 0, 0);
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[j].y, b[n].y, acc[n], 0, 0, 0);
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[j].z, b[n].z, acc[n], 0, 0, 0);
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[j].w, b[n].w, acc[n], 0, 0, 0);
                }
            }
            if (!have_next) break;
            store_B(buf ^ 1);
            __syncthreads();
            buf ^= 1;
            k = kn;
            c = cn;
            act_cur = act_nxt;
#pragma unroll
            for (int j = 0; j < NJ; ++j) a_cur[j] = a_nxt[j];
        }
    }
    // epilogue: D row = 4q + reg, col = r
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = row0 + wrow + 4 * q + reg;
        if (row < n_rows) {
#pragma unroll
            for (int n = 0; n < NB; ++n)
                if (col0 + 16 * n + r < cout) out[(size_t)row * cout + col0 + 16 * n + r] = acc[n][reg];
        }
    }
}

template <int NB, int KC>
static void launch_conv_lk(dim3 grid, hipStream_t st, const float *in, int64_t n_in, int cin, const float *wt, int cout,
                           const int32_t *nbr, int64_t ld, int64_t n_rows, int K, int kflip, float *out) {
    const size_t lds = (size_t)2 * 16 * NB * (KC + 8) * 4 + (size_t)32 * 64 * 4 + 2 * 4 * 4;
    static_assert((size_t)2 * 16 * NB * (KC + 8) * 4 + 32 * 64 * 4 + 32 <= 65536, "conv_lk: LDS above 64 KiB");
    hipLaunchKernelGGL((conv_lk_kernel<NB, KC>), grid, dim3(256), lds, st, in, n_in, cin, wt, cout, nbr, ld, n_rows, K, kflip,
                       out);
}

// 16-column blocks per workgroup: all of them up to 64 columns, else the divisor of the block count that leaves no ragged tile
static int lk_pick_nb(int c16) {
    if (c16 <= 4) return c16;
    if (c16 % 4 == 0) return 4;
    if (c16 % 3 == 0) return 3;
    return 4;   // ragged last tile is masked
}

}  // namespace u2mkd

using namespace u2mkd;

extern "C" {

int32_t u2mkd_conv_lk_supported(int32_t cin, int32_t cout, int32_t k) {
    return cin > 0 && cin % 4 == 0 && cout > 0 && k >= 1 && k <= kLkMaxVolume;
}

int u2mkd_conv_forward_lk(const float *in, int64_t n_in, int32_t cin, const float *wt, int32_t cout, const int32_t *nbr,
                          int64_t ld, int64_t n_rows, int32_t k, int32_t kflip, float *out, u2mkd_stream_t s) {
    if (n_rows == 0) return 0;
    U2_REQUIRE(in && wt && nbr && out, "u2mkd_conv_forward_lk: null pointer");
    U2_REQUIRE(cin > 0 && cin % 4 == 0, "u2mkd_conv_forward_lk: cin=%d must be a positive multiple of 4", cin);
    U2_REQUIRE(cout > 0, "u2mkd_conv_forward_lk: cout=%d must be positive", cout);
    U2_REQUIRE(k >= 1 && k <= kLkMaxVolume, "u2mkd_conv_forward_lk: kernel volume %d not in 1..%d", k, kLkMaxVolume);
    U2_REQUIRE(n_rows > 0 && n_in >= 0 && ld >= n_rows, "u2mkd_conv_forward_lk: n_rows=%lld n_in=%lld ld=%lld", (long long)n_rows,
               (long long)n_in, (long long)ld);
    U2_REQUIRE(kflip == 0 || kflip == 1, "u2mkd_conv_forward_lk: kflip must be 0 or 1");
    const int c16 = (cout + 15) / 16;
    const int nb = lk_pick_nb(c16);
    // channels per step: the whole row of a narrow layer (the 4-channel stem: one of four product steps is not zeros), 64 where
    // the row is a multiple of it, else 32 -- as conv_os2 takes them
    const int kc = cin <= 16 ? 16 : (cin % 64 == 0 ? 64 : 32);
    const int64_t tiles = ceil_div(n_rows, 64);
    U2_REQUIRE(tiles <= 0x7fffffff, "u2mkd_conv_forward_lk: %lld rows are too many", (long long)n_rows);
    dim3 grid((unsigned)tiles, (unsigned)ceil_div(c16, nb));
    hipStream_t st = as_stream(s);
#define U2_LK(NB_, KC_) launch_conv_lk<NB_, KC_>(grid, st, in, n_in, cin, wt, cout, nbr, ld, n_rows, k, kflip, out)
#define U2_LK_KC(NB_)                          \
    do {                                       \
        if (kc == 16) U2_LK(NB_, 16);          \
        else if (kc == 32) U2_LK(NB_, 32);     \
        else U2_LK(NB_, 64);                   \
    } while (0)
    switch (nb) {
        case 1: U2_LK_KC(1); break;
        case 2: U2_LK_KC(2); break;
        case 3: U2_LK_KC(3); break;
        default: U2_LK_KC(4); break;
    }
#undef U2_LK_KC
#undef U2_LK
    return check_launch("u2mkd_conv_forward_lk");
}

}  // extern "C"
