// emg_neigh.hip — embedding-space discovery: the radius join behind find_duplicates and the unit-norm copy the cosine
// metric works on (AmpliGraph 1.x discovery API: find_duplicates / find_nearest_neighbours).
//
// DISTANCES (the contract of emgraph_amd/discovery.py): l2 is sqrtf of the k-ordered chain fmaf(d, d, acc), d = a_k - b_k
// — the bits of -chain_score(EMG_TRANSE_L2), so a pair has the distance the exact 1-vs-all kernels give it; cosine is
// 1 - dot with dot the k-ordered chain fmaf(a_k, b_k, acc) over rows emg_rows_normalize made.  Distance and comparison are
// unquantised f32 (emg_eval_count compares int32(score * 1e5): it cannot find "within 1e-7").
//
// RADIUS JOIN (rows_within_kernel): a workgroup owns 64 rows of A and streams every row of B past them, 64 at a time, k tiles
// of both staged in LDS (the main loop of topn_transe_kernel: 4 x 4 chains per thread; emg_rowtile.hpp, shared with the link
// pass of emg_cluster.hip).  A row's count and its nearest
// other row stay in registers over the whole stream and meet in LDS once, at the end: no global atomic, one plain store
// per output.  Pairs within the radius are rare; a wave that found some reserves room for all of them with ONE add on
// pair_count and stores them behind each other.  Nothing is stored at or past pairs_capacity.
#include "emg_rowtile.hpp"

#pragma clang fp contract(off)

namespace emg {
namespace {

struct WithinParams {
    const float* A; int64_t n_a, ld_a;
    const float* B; int64_t n_b, ld_b;
    int32_t k_int; int64_t self_offset; float radius;
    int32_t* count; float* nn_dist; int32_t* nn_id;
    unsigned long long* pairs; int64_t cap; unsigned long long* pair_count;
};

template <int METRIC>
__global__ __launch_bounds__(256) void rows_within_kernel(const WithinParams P) {
    __shared__ __attribute__((aligned(16))) float As[TK * TA];
    __shared__ __attribute__((aligned(16))) float Bs[TK * TB];
    __shared__ int cnt_s[TA];
    __shared__ unsigned long long key_s[TA];

    const int tid = threadIdx.x, lane = tid & 63;
    const int tq = tid & 15, te = tid >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * TA;

    if (tid < TA) { cnt_s[tid] = 0; key_s[tid] = KEY_NONE; }

    int cnt[4] = {0, 0, 0, 0};
    unsigned long long best[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};

    // the tile loop is emg_rowtile.hpp's; what follows is this kernel's share of a tile
    rowtile_stream<METRIC>(P.A, P.n_a, P.ld_a, P.B, P.n_b, P.ld_b, P.k_int, row0, (P.n_b + TB - 1) / TB, As, Bs,
                           [&](int64_t tile, const float (&acc)[16]) __attribute__((always_inline)) {
        unsigned hit = 0u;
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int64_t i = row0 + 4 * tq + x, j = tile * TB + 4 * te + y;
                const float d = rowtile_distance<METRIC>(acc[4 * x + y]);
                const bool other = i < P.n_a && j < P.n_b && !(P.self_offset >= 0 && j == P.self_offset + i);
                if (other && d <= P.radius) { ++cnt[x]; hit |= 1u << (4 * x + y); }
                if (other && d == d) best[x] = min(best[x], dist_key(d, j));
            }
        if (P.pairs && __ballot(hit != 0u)) {   // wave-uniform; every lane of the workgroup reaches the ballot
            const int n = __popc(hit);
            int incl = n;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            const int total = __shfl(incl, 63);
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(P.pair_count, (unsigned long long)total);
            base = __shfl(base, 0);
            unsigned long long pos = base + (unsigned long long)(incl - n);
            while (hit) {
                const int r = __ffs(hit) - 1;
                hit &= hit - 1u;
                const int64_t i = row0 + 4 * tq + (r >> 2), j = tile * TB + 4 * te + (r & 3);
                if (pos < (unsigned long long)P.cap) P.pairs[pos] = ((unsigned long long)i << 32) | (unsigned long long)j;
                ++pos;
            }
        }
    });
    __syncthreads();   // (also for n_b == 0: the LDS records are initialised)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        if (cnt[x]) atomicAdd(&cnt_s[4 * tq + x], cnt[x]);
        if (best[x] != KEY_NONE) atomicMin(&key_s[4 * tq + x], best[x]);
    }
    __syncthreads();
    if (tid < TA && row0 + tid < P.n_a) {
        const unsigned long long key = key_s[tid];
        P.count[row0 + tid] = cnt_s[tid];
        P.nn_dist[row0 + tid] = key == KEY_NONE ? INFINITY : key_dist(key);
        P.nn_id[row0 + tid] = key == KEY_NONE ? -1 : (int32_t)(uint32_t)key;
    }
}

// pair_count[0] counted every pair found; what was written is the part that fitted
__global__ void pairs_finish_kernel(unsigned long long* pair_count, int64_t cap) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && pair_count[0] > (unsigned long long)cap) {
        pair_count[0] = (unsigned long long)cap;
        pair_count[1] = 1ull;
    }
}

// One thread per row: the chain sum of squares in k order, then every element divided by its square root.
__global__ __launch_bounds__(256) void rows_normalize_kernel(const float* __restrict__ src, int64_t n_rows, int64_t ld_src, int32_t k_int,
                                                             float* __restrict__ dst, int64_t ld_dst) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const float* s = src + row * ld_src;
    float* d = dst + row * ld_dst;
    float ss = 0.f;
    for (int k = 0; k < k_int; ++k) ss = __fmaf_rn(s[k], s[k], ss);
    const float norm = sqrtf(ss);
    for (int k = 0; k < k_int; ++k) d[k] = ss > 0.f ? __fdiv_rn(s[k], norm) : 0.f;   // an all-zero row stays zero
}

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" int emg_rows_normalize(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int, float* dst, int64_t ld_dst,
                                  void* stream) {
    EMG_REQUIRE(n_rows >= 0 && k_int > 0 && ld_src >= k_int && ld_dst >= k_int, "emg_rows_normalize: bad sizes");
    if (n_rows == 0) return EMG_OK;
    EMG_REQUIRE(src && dst, "emg_rows_normalize: null pointer");
    EMG_REQUIRE(cdiv(n_rows, 256) < ((int64_t)1 << 31), "emg_rows_normalize: grid too large");
    hipLaunchKernelGGL(rows_normalize_kernel, dim3((unsigned)cdiv(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, src, n_rows, ld_src,
                       k_int, dst, ld_dst);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_rows_within(int metric, const float* A, int64_t n_a, int64_t ld_a, const float* B, int64_t n_b, int64_t ld_b,
                               int32_t k_int, int64_t self_offset, float radius, int32_t* count, float* nn_dist, int32_t* nn_id,
                               uint64_t* pairs, int64_t pairs_capacity, uint64_t* pair_count, void* stream) {
    EMG_REQUIRE(metric == EMG_METRIC_L2 || metric == EMG_METRIC_COSINE, "emg_rows_within: unknown metric %d", metric);
    EMG_REQUIRE(n_a >= 0 && n_b >= 0 && n_a <= INT32_MAX && n_b <= INT32_MAX && k_int > 0 && ld_a >= k_int && ld_b >= k_int &&
                pairs_capacity >= 0, "emg_rows_within: bad sizes");
    EMG_REQUIRE(self_offset >= -1 && (self_offset < 0 || self_offset + n_a <= n_b), "emg_rows_within: A is not rows [%lld, %lld) of B",
                (long long)self_offset, (long long)(self_offset + n_a));
    EMG_REQUIRE(radius == radius, "emg_rows_within: the radius is NaN");
    EMG_REQUIRE(!pairs || pair_count, "emg_rows_within: pairs without pair_count");
    EMG_REQUIRE(((reinterpret_cast<uintptr_t>(pairs) | reinterpret_cast<uintptr_t>(pair_count)) & 7u) == 0,
                "emg_rows_within: pairs and pair_count must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (pair_count) EMG_HIP(hipMemsetAsync(pair_count, 0, 2 * sizeof(uint64_t), st));
    if (n_a == 0) return EMG_OK;
    EMG_REQUIRE(A && count && nn_dist && nn_id && (n_b == 0 || B), "emg_rows_within: null pointer");
    WithinParams P{};
    P.A = A; P.n_a = n_a; P.ld_a = ld_a; P.B = B; P.n_b = n_b; P.ld_b = ld_b; P.k_int = k_int; P.self_offset = self_offset;
    P.radius = radius; P.count = count; P.nn_dist = nn_dist; P.nn_id = nn_id;
    P.pairs = reinterpret_cast<unsigned long long*>(pairs); P.cap = pairs_capacity;
    P.pair_count = reinterpret_cast<unsigned long long*>(pair_count);
    void (*fn)(const WithinParams) = metric == EMG_METRIC_L2 ? rows_within_kernel<0> : rows_within_kernel<1>;
    hipLaunchKernelGGL(fn, dim3((unsigned)cdiv(n_a, TA)), dim3(256), 0, st, P);
    EMG_LAUNCH_CHECK();
    if (pairs) {
        hipLaunchKernelGGL(pairs_finish_kernel, dim3(1), dim3(64), 0, st, P.pair_count, pairs_capacity);
        EMG_LAUNCH_CHECK();
    }
    return EMG_OK;
}
