// emg_rowtile.hpp — the tile stream of the all-pairs row kernels (emg_neigh.hip: the radius join; emg_cluster.hip: DBSCAN's
// link pass).  A workgroup of 256 threads owns TA = 64 rows of A and streams rows of B past them TB = 64 at a time, k tiles
// of TK = 32 of both staged in LDS, 4 x 4 chains per thread (the main loop of topn_transe_kernel).  The loop exists ONCE:
// every kernel that includes this header forms a pair's chain with the same steps in the same order, so a pair has the same
// distance bits in all of them.
#pragma once
#include "emg_chain.hpp"

#pragma clang fp contract(off)

namespace emg {

constexpr int TA = 64, TB = 64, TK = 32;

// The distance of EMG_METRIC_L2 (METRIC 0) / EMG_METRIC_COSINE (METRIC 1) from a finished chain.
template <int METRIC>
__device__ __forceinline__ float rowtile_distance(float acc) {
    return METRIC == 0 ? sqrtf(acc) : __fsub_rn(1.0f, acc);
}

// The nearest-row record of the kernels that keep a minimum over the stream (emg_neigh.hip, emg_kmeans.hip):
constexpr unsigned long long KEY_NONE = ~0ull;   // no candidate yet

// (distance, id) as one integer whose order is ascending distance, then ascending id (the distance is no NaN)
__device__ __forceinline__ unsigned long long dist_key(float d, int64_t j) {
    const uint32_t u = __float_as_uint(d);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)k << 32) | (uint32_t)j;
}

__device__ __forceinline__ float key_dist(unsigned long long key) {
    const uint32_t k = (uint32_t)(key >> 32);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Streams the B tiles [0, n_tiles) past the workgroup's rows [row0, row0 + TA) of A and calls epi(tile, acc) once per tile
// with the thread's 16 finished chains: acc[4 x + y] belongs to A row row0 + 4 tq + x and B row tile * TB + 4 te + y,
// tq = tid & 15, te = tid >> 4 (rows past the tables' ends are clamped copies of the last row: the epilogue masks them).
// As, Bs: TK * TA and TK * TB floats of LDS, 16-byte aligned.  Every thread of the workgroup must call this (barriers inside);
// n_tiles is uniform.  LDS the caller initialised before the call is visible to all threads once the first tile's barrier has
// passed, i.e. inside epi.
template <int METRIC, class Epilogue>
__device__ __forceinline__ void rowtile_stream(const float* A, int64_t n_a, int64_t ld_a, const float* B, int64_t n_b, int64_t ld_b,
                                               int32_t k_int, int64_t row0, int64_t n_tiles, float* As, float* Bs, Epilogue&& epi) {
    const int tid = threadIdx.x;
    const int tq = tid & 15, te = tid >> 4;
    const int lrow = tid & 63, lkq = tid >> 6;  // loader: row lrow, 4-float slots lkq and lkq+4 of the k-tile
    const float* aptr = A + min(row0 + lrow, n_a - 1) * ld_a;
    for (int64_t tile = 0; tile < n_tiles; ++tile) {
        const float* bptr = B + min(tile * TB + lrow, n_b - 1) * ld_b;
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < k_int; k0 += TK) {
            float av[2][4], bv[2][4];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kb = k0 + 4 * (lkq + 4 * h);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    av[h][c] = kb + c < k_int ? aptr[kb + c] : 0.f;
                    bv[h][c] = kb + c < k_int ? bptr[kb + c] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int kl = 4 * (lkq + 4 * h) + c;
                    As[kl * TA + lrow] = av[h][c];
                    Bs[kl * TB + lrow] = bv[h][c];
                }
            __syncthreads();
            const int kn = min(TK, k_int - k0);   // the chain stops at k_int: exactly chain_score's steps
            for (int k = 0; k < kn; ++k) {
                const float4 a4 = *reinterpret_cast<const float4*>(&As[k * TA + 4 * tq]);
                const float4 b4 = *reinterpret_cast<const float4*>(&Bs[k * TB + 4 * te]);
                const float a[4] = {a4.x, a4.y, a4.z, a4.w};
                const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[4 * x + y] = chain_step<METRIC == 0 ? 2 : 0>(a[x], b[y], acc[4 * x + y]);
            }
        }
        epi(tile, acc);
    }
}

}  // namespace emg
