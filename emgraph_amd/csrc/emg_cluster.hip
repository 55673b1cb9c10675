// emg_cluster.hip — embedding-space clustering: an exact DBSCAN on the device (AmpliGraph 1.x find_clusters with its default
// algorithm; DESIGN.md 4.4 "Clusters").  DBSCAN is a radius join plus connected components; the join is emg_neigh.hip's,
// with its distances (unquantised f32, d <= eps inclusive, bit-symmetric in (i, j)).
//
//   count   emg_rows_within without pairs: |N(i)| - 1 for every row; row i is core iff count[i] + 1 >= min_samples.
//   link    the same tile stream (emg_rowtile.hpp) once more.  A hit between two core rows unions them in parent[] (unite()
//           below: agent-scope compare-and-swap only); a hit of a non-core row i on a core row j appends j to row i's border
//           list — at most min_samples - 2 entries, a fixed stride per row, the cursor in LDS because the workgroup owns its
//           64 rows of A for the whole stream: no global atomic for the lists.
//   finish  four small launches behind kernel boundaries (plain loads): every row's root, an exact integer scan of the core
//           roots (a cluster's number is the count of core roots with a lower index), the labels, and info.
//
// Every component of the core rows ends as ONE tree whose root is its lowest row index, so the numbering "ascending lowest
// core row" falls out of the scan, and a border row's label is the minimum over its list: the labels are fully determined
// and equal sklearn.cluster.DBSCAN.fit_predict's.
#include "emg_rowtile.hpp"

#pragma clang fp contract(off)

namespace emg {
namespace {

constexpr int FB = 1024;   // rows per workgroup of the finish kernels (256 threads x 4)

static inline size_t r16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// a non-core row has fewer than min_samples - 1 other rows within eps, and there are only n - 1 other rows
static inline int64_t border_stride(int64_t n, int32_t min_samples) {
    const int64_t s = (int64_t)min_samples - 2;
    return s < 0 ? 0 : (s < n - 1 ? s : (n > 0 ? n - 1 : 0));
}

struct Workspace {
    int64_t* stats;   // [2]: the longest parent chain the finish walked, 0
    int32_t* count; float* nn_dist; int32_t* nn_id;   // the count pass's outputs
    int32_t *parent, *root, *rank, *border_n;          // [n] each
    int32_t *bsum, *bmax, *bnoise;                     // [cdiv(n, FB)] each
    int32_t* lists;                                    // [n, stride]
    size_t bytes;                                      // SIZE_MAX: not representable
};

static Workspace carve(void* ws, int64_t n, int32_t min_samples) {
    Workspace W{};
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += r16(bytes); return q; };
    const size_t nn = (size_t)n, nblk = (size_t)cdiv(n, FB), stride = (size_t)border_stride(n, min_samples);
    W.stats = reinterpret_cast<int64_t*>(take(16));
    W.count = reinterpret_cast<int32_t*>(take(4 * nn));
    W.nn_dist = reinterpret_cast<float*>(take(4 * nn));
    W.nn_id = reinterpret_cast<int32_t*>(take(4 * nn));
    W.parent = reinterpret_cast<int32_t*>(take(4 * nn));
    W.root = reinterpret_cast<int32_t*>(take(4 * nn));
    W.rank = reinterpret_cast<int32_t*>(take(4 * nn));
    W.border_n = reinterpret_cast<int32_t*>(take(4 * nn));
    W.bsum = reinterpret_cast<int32_t*>(take(4 * nblk));
    W.bmax = reinterpret_cast<int32_t*>(take(4 * nblk));
    W.bnoise = reinterpret_cast<int32_t*>(take(4 * nblk));
    if (stride != 0 && nn > (((size_t)1 << 60) / stride)) { W.bytes = SIZE_MAX; return W; }   // n * stride * 4 must not wrap
    W.lists = reinterpret_cast<int32_t*>(take(4 * nn * stride));
    W.bytes = off;
    return W;
}

__global__ __launch_bounds__(256) void dbscan_init_kernel(const int32_t* __restrict__ count, int64_t n, int32_t min_samples,
                                                          uint8_t* __restrict__ is_core, int32_t* __restrict__ parent) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    is_core[x] = (int64_t)count[x] + 1 >= (int64_t)min_samples ? 1 : 0;   // the row itself counts (scikit-learn's rule)
    parent[x] = (int32_t)x;
}

// UNION of the trees that hold a and b; returns a row that is an ancestor (or the row itself) of BOTH afterwards.
//
// parent[] starts as the identity (a previous launch) and is changed in this launch ONLY by the compare-and-swap below, which
// replaces parent[a] == a by b < a: a word is written at most once (afterwards it is no root and never matches again), and
// parent[x] <= x always holds, so there is no cycle.  Every value the loop continues with is the return value of that
// agent-scope atomic — the word's true content at the time of the atomic — never a plain load: per-XCD L2s are not coherent
// and a CU's L1 is never refreshed, so a loop over plain loads could spin on a stale line for ever.
// Termination: a failed swap returns old = parent[a] != a, hence old < a; the loop goes on with (old, b) in place of (a, b)
// where a = max(a, b) — the maximum of the pair falls strictly in every iteration and is >= 0: at most n iterations.
// Result: the loop ends either with a == b (both climbs met: a common ancestor) or by hooking the ROOT a under b (b is then
// an ancestor of both).  Only roots are hooked, and under a lower index, so the lowest row of a component is never hooked:
// when all edges are in, every component is one tree rooted at its lowest row.
// Callers may start from any ancestor of a row in place of the row (unite's own result for an earlier edge of that row): the
// trees joined are the same.
__device__ __forceinline__ int unite(int32_t* parent, int a, int b) {
    for (;;) {
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(&parent[a], a, b);   // hook a under b only while a is a root
        if (old == a) return b;
        a = old;                                        // otherwise climb with the value the atomic returned
    }
}

struct LinkParams {
    const float* X; int64_t n, ld; int32_t k_int; float eps;
    const uint8_t* is_core; int32_t* parent; int32_t* lists; int32_t* border_n; int64_t stride;
};

template <int METRIC>
__global__ __launch_bounds__(256) void dbscan_link_kernel(const LinkParams P) {
    __shared__ __attribute__((aligned(16))) float As[TK * TA];
    __shared__ __attribute__((aligned(16))) float Bs[TK * TB];
    __shared__ int cur_s[TA];   // entries in each owned row's border list

    const int tid = threadIdx.x;
    const int tq = tid & 15, te = tid >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * TA;

    if (tid < TA) cur_s[tid] = 0;
    bool core_i[4];
    int rep_i[4];   // an ancestor of row i from the unions so far: later edges of the row start their climb there
    int noncore = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int64_t i = row0 + 4 * tq + x;
        core_i[x] = i < P.n && P.is_core[i] != 0;
        rep_i[x] = (int)i;
        noncore |= i < P.n && !core_i[x];
    }
    // core rows only need the rows below them (an edge is handled once, from its higher end); a border list needs every row
    const int64_t n_tiles = __syncthreads_or(noncore) ? (P.n + TB - 1) / TB : (int64_t)blockIdx.x + 1;

    rowtile_stream<METRIC>(P.X, P.n, P.ld, P.X, P.n, P.ld, P.k_int, row0, n_tiles, As, Bs,
                           [&](int64_t tile, const float (&acc)[16]) __attribute__((always_inline)) {
        int rep_j[4];
#pragma unroll
        for (int y = 0; y < 4; ++y) rep_j[y] = (int)(tile * TB + 4 * te + y);
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int64_t i = row0 + 4 * tq + x, j = tile * TB + 4 * te + y;
                const float d = rowtile_distance<METRIC>(acc[4 * x + y]);
                if (i < P.n && j < P.n && i != j && d <= P.eps && P.is_core[j] != 0) {
                    if (core_i[x]) {
                        if (j < i) rep_i[x] = rep_j[y] = unite(P.parent, rep_i[x], rep_j[y]);
                    } else {
                        const int slot = atomicAdd(&cur_s[4 * tq + x], 1);   // LDS
                        if (slot < P.stride) P.lists[i * P.stride + slot] = (int32_t)j;
                    }
                }
            }
    });
    __syncthreads();
    if (tid < TA && row0 + tid < P.n) P.border_n[row0 + tid] = (int32_t)min((int64_t)cur_s[tid], P.stride);
}

// exclusive scan of one int per thread over a workgroup of 256; `total` is the workgroup's sum.  s_w: 4 ints of LDS.
__device__ __forceinline__ int block_scan_excl(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    __syncthreads();   // (s_w may still be read from the previous call)
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < w) base += s_w[q];
        total += s_w[q];
    }
    return base + incl - v;
}

// root[x] = the fixed point of parent; per workgroup: the core roots, the noise rows and the longest chain walked
__global__ __launch_bounds__(256) void dbscan_roots_kernel(const int32_t* __restrict__ parent, const uint8_t* __restrict__ is_core,
                                                           const int32_t* __restrict__ border_n, int64_t n,
                                                           int32_t* __restrict__ root, int32_t* __restrict__ bsum,
                                                           int32_t* __restrict__ bmax, int32_t* __restrict__ bnoise) {
    __shared__ int s_sum, s_max, s_noise;
    if (threadIdx.x == 0) { s_sum = 0; s_max = 0; s_noise = 0; }
    __syncthreads();
    int sum = 0, longest = 0, noise = 0;
#pragma unroll
    for (int e = 0; e < FB / 256; ++e) {
        const int64_t x = (int64_t)blockIdx.x * FB + e * 256 + threadIdx.x;
        if (x >= n) break;
        int r = (int)x, steps = 0;
        for (int p = parent[r]; p != r; p = parent[r]) { r = p; ++steps; }   // parent[r] < r: ends at a root
        root[x] = r;
        const bool core = is_core[x] != 0;
        sum += core && r == (int)x;
        noise += !core && border_n[x] == 0;
        longest = max(longest, steps);
    }
    if (sum) atomicAdd(&s_sum, sum);
    if (noise) atomicAdd(&s_noise, noise);
    if (longest) atomicMax(&s_max, longest);
    __syncthreads();
    if (threadIdx.x == 0) { bsum[blockIdx.x] = s_sum; bmax[blockIdx.x] = s_max; bnoise[blockIdx.x] = s_noise; }
}

// one workgroup: bsum becomes its own exclusive scan; info = {clusters, noise rows}; stats[0] = the longest chain
__global__ __launch_bounds__(256) void dbscan_scan_kernel(int32_t* __restrict__ bsum, const int32_t* __restrict__ bmax,
                                                          const int32_t* __restrict__ bnoise, int64_t nblk,
                                                          int64_t* __restrict__ info, int64_t* __restrict__ stats) {
    __shared__ int s_w[4];
    __shared__ int s_max;
    __shared__ unsigned long long s_noise;
    if (threadIdx.x == 0) { s_max = 0; s_noise = 0ull; }
    int carry = 0, longest = 0;
    unsigned long long noise = 0ull;
    for (int64_t c0 = 0; c0 < nblk; c0 += 256) {
        const int64_t b = c0 + threadIdx.x;
        const int v = b < nblk ? bsum[b] : 0;
        int total;
        const int excl = block_scan_excl(v, s_w, total);
        if (b < nblk) {
            bsum[b] = carry + excl;
            longest = max(longest, bmax[b]);
            noise += (unsigned long long)bnoise[b];
        }
        carry += total;
    }
    __syncthreads();
    if (noise) atomicAdd(&s_noise, noise);
    if (longest) atomicMax(&s_max, longest);
    __syncthreads();
    if (threadIdx.x == 0) {
        info[0] = (int64_t)carry;
        info[1] = (int64_t)s_noise;
        stats[0] = (int64_t)s_max;
        stats[1] = 0;
    }
}

// rank[x] = the core roots with a lower index than x (a thread scans 4 consecutive rows)
__global__ __launch_bounds__(256) void dbscan_rank_kernel(const int32_t* __restrict__ root, const uint8_t* __restrict__ is_core,
                                                          const int32_t* __restrict__ bsum, int64_t n, int32_t* __restrict__ rank) {
    __shared__ int s_w[4];
    const int64_t x0 = (int64_t)blockIdx.x * FB + 4 * threadIdx.x;
    int flag[4], mine = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t x = x0 + e;
        flag[e] = x < n && is_core[x] != 0 && root[x] == (int32_t)x;
        mine += flag[e];
    }
    int total;
    int run = bsum[blockIdx.x] + block_scan_excl(mine, s_w, total);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (x0 + e < n) rank[x0 + e] = run;
        run += flag[e];
    }
}

// core rows take their cluster's number, the others the lowest number among their border list, -1 without one
__global__ __launch_bounds__(256) void dbscan_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ rank,
                                                           const uint8_t* __restrict__ is_core, const int32_t* __restrict__ border_n,
                                                           const int32_t* __restrict__ lists, int64_t stride, int64_t n,
                                                           int32_t* __restrict__ labels) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    if (is_core[x]) { labels[x] = rank[root[x]]; return; }
    int best = INT32_MAX;
    const int m = border_n[x];
    for (int t = 0; t < m; ++t) best = min(best, rank[root[lists[x * stride + t]]]);
    labels[x] = m ? best : -1;
}

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" size_t emg_rows_dbscan_ws_bytes(int64_t n, int32_t min_samples) {
    if (n < 0 || n > INT32_MAX || min_samples < 1) return 0;
    return carve(nullptr, n, min_samples).bytes;
}

extern "C" int emg_rows_dbscan(int metric, const float* X, int64_t n, int64_t ld, int32_t k_int, float eps, int32_t min_samples,
                               int32_t* labels, uint8_t* is_core, int64_t* info, void* ws, size_t ws_bytes, void* stream) {
    EMG_REQUIRE(metric == EMG_METRIC_L2 || metric == EMG_METRIC_COSINE, "emg_rows_dbscan: unknown metric %d", metric);
    EMG_REQUIRE(n >= 0 && n <= INT32_MAX && k_int > 0 && ld >= k_int, "emg_rows_dbscan: bad sizes");
    EMG_REQUIRE(eps == eps && eps >= 0.f, "emg_rows_dbscan: eps must be a number >= 0");
    EMG_REQUIRE(min_samples >= 1, "emg_rows_dbscan: min_samples %d < 1", min_samples);
    const Workspace W = carve(ws, n, min_samples);
    EMG_REQUIRE(W.bytes != SIZE_MAX && ws_bytes >= W.bytes, "emg_rows_dbscan: the workspace holds %llu bytes, %llu are needed",
                (unsigned long long)ws_bytes, (unsigned long long)W.bytes);
    EMG_REQUIRE(ws && aligned16(ws), "emg_rows_dbscan: the workspace must be 16-byte aligned");
    EMG_REQUIRE(info && (reinterpret_cast<uintptr_t>(info) & 7u) == 0, "emg_rows_dbscan: info must be an 8-byte aligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        EMG_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int64_t), st));
        return EMG_OK;
    }
    EMG_REQUIRE(X && labels && is_core, "emg_rows_dbscan: null pointer");

    // (a) count: the join without pairs
    const int rc = emg_rows_within(metric, X, n, ld, X, n, ld, k_int, 0, eps, W.count, W.nn_dist, W.nn_id, nullptr, 0, nullptr, stream);
    if (rc != EMG_OK) return rc;
    const unsigned g256 = (unsigned)cdiv(n, 256), gfb = (unsigned)cdiv(n, FB);
    hipLaunchKernelGGL(dbscan_init_kernel, dim3(g256), dim3(256), 0, st, W.count, n, min_samples, is_core, W.parent);
    EMG_LAUNCH_CHECK();

    // (b) link
    LinkParams P{};
    P.X = X; P.n = n; P.ld = ld; P.k_int = k_int; P.eps = eps; P.is_core = is_core; P.parent = W.parent; P.lists = W.lists;
    P.border_n = W.border_n; P.stride = border_stride(n, min_samples);
    void (*link)(const LinkParams) = metric == EMG_METRIC_L2 ? dbscan_link_kernel<0> : dbscan_link_kernel<1>;
    hipLaunchKernelGGL(link, dim3((unsigned)cdiv(n, TA)), dim3(256), 0, st, P);
    EMG_LAUNCH_CHECK();

    // (c) finish
    hipLaunchKernelGGL(dbscan_roots_kernel, dim3(gfb), dim3(256), 0, st, W.parent, is_core, W.border_n, n, W.root, W.bsum, W.bmax,
                       W.bnoise);
    EMG_LAUNCH_CHECK();
    hipLaunchKernelGGL(dbscan_scan_kernel, dim3(1), dim3(256), 0, st, W.bsum, W.bmax, W.bnoise, (int64_t)gfb, info, W.stats);
    EMG_LAUNCH_CHECK();
    hipLaunchKernelGGL(dbscan_rank_kernel, dim3(gfb), dim3(256), 0, st, W.root, is_core, W.bsum, n, W.rank);
    EMG_LAUNCH_CHECK();
    hipLaunchKernelGGL(dbscan_label_kernel, dim3(g256), dim3(256), 0, st, W.root, W.rank, is_core, W.border_n, W.lists, P.stride, n,
                       labels);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
