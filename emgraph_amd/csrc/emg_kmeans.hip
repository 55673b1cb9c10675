// emg_kmeans.hip — embedding-space clustering: Lloyd's k-means and k-means++ seeding on the device (the estimator
// emgraph_amd.discovery.KMeans behind find_clusters; DESIGN.md 4.4 "k-means").  The contract is restated in
// include/emgraph_hip.h; what this file adds to it is HOW the fixed orders are produced.
//
// ONE LLOYD RUN (emg_rows_kmeans) is a fixed list of launches on the stream, no host read in between.  A 48-byte State record
// in the workspace carries {done, n_iter, converged, changed, tol_abs, shift}; every launch of an iteration starts with
// `if (st->done) return` (a plain load: the flag was written by an earlier launch), so the iterations enqueued past the stop
// cost one empty launch each.
//
//   tolerance  (max_iter > 0) column means and variances of X in f64, two-pass, over chunks of 256 consecutive rows:
//              tol_abs = tol * mean over columns of var (scikit-learn's _tolerance)
//   assign     the tile stream of emg_rowtile.hpp with B = the centres and the (distance, id) minimum of emg_rows_within:
//              label = the lowest j among the nearest centres, -1 if every distance is a NaN; a workgroup that changed a label
//              raises State::changed
//   per iteration:
//     hist     a workgroup per 256 consecutive rows: every row's rank among the rows of its block with the same label, and
//              the block's count per label (cnt[block][label])
//     colscan  a thread per label: cnt[.][label] becomes its exclusive scan over the blocks; count[label]
//     starts   one workgroup: start[] = exclusive scan of count[], cstart[] = exclusive scan of the chunks ceil(count / 256)
//     scatter  order[start[label] + cnt[block][label] + rank] = row: a STABLE counting sort — the members of a cluster in
//              ascending row order, which no atomic's arrival order can change (the only atomics here are on integers)
//     chunks   a workgroup per chunk of 256 members: a thread per column adds (double)x of the chunk's rows one after the
//              other, in member order
//     centres  a workgroup per cluster: a thread per column adds the cluster's chunk sums one after the other, divides by the
//              count, rounds to f32, and adds the squared move to the cluster's share of the shift; an empty cluster is left
//     assign   as above, against the new centres
//     decide   shift = sum of the clusters' shares (fixed order); ++n_iter; done when no label changed or shift <= tol_abs
//   inertia    sum of (double)d * (double)d over the labelled rows: a fixed tree per 256 rows, the blocks in a fixed order
//
// No floating-point atomic anywhere: two runs give the same bits.
#include "emg_rowtile.hpp"

#pragma clang fp contract(off)

namespace emg {
namespace {

constexpr int CH = 256;   // rows per block of the counting sort = members per chunk of the update = rows per seeding segment

struct State {
    int32_t done, n_iter, converged, changed;
    double tol_abs, shift, inertia, reserved;
};
static_assert(sizeof(State) == 48, "State layout");

static inline size_t r16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

struct Workspace {
    State* st;
    float* dist;                          // [n]   distance to the assigned centre
    int32_t *rank, *order;                // [n]   rank inside (block, label); rows sorted by label
    int32_t* cnt;                         // [nblk, C]
    int32_t *count, *start, *cstart;      // [C], [C + 1], [C + 1]
    double *shiftj, *colmean, *colvar;    // [C], [k], [k]
    double* partial;                      // [nblk + C, k]  chunk sums (an upper bound of the chunks: sum ceil(count_j / 256))
    double* ipart;                        // [nblk]
    float* seed_m;                        // [n]   seeding: distance to the nearest centre chosen so far
    double* segt;                         // [nblk] seeding: segment totals
    size_t bytes;                         // SIZE_MAX: not representable
};

static Workspace carve(void* ws, int64_t n, int64_t C, int32_t k) {
    Workspace W{};
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += r16(bytes); return q; };
    const size_t nn = (size_t)n, cc = (size_t)C, kk = (size_t)k, nblk = (size_t)cdiv(n, CH);
    // nblk * C * 4 < 2^58; (nblk + C) * k * 8 must not wrap
    if ((nblk + cc) > (((size_t)1 << 60) / kk)) { W.bytes = SIZE_MAX; return W; }
    W.st = reinterpret_cast<State*>(take(64));
    W.dist = reinterpret_cast<float*>(take(4 * nn));
    W.rank = reinterpret_cast<int32_t*>(take(4 * nn));
    W.order = reinterpret_cast<int32_t*>(take(4 * nn));
    W.cnt = reinterpret_cast<int32_t*>(take(4 * nblk * cc));
    W.count = reinterpret_cast<int32_t*>(take(4 * cc));
    W.start = reinterpret_cast<int32_t*>(take(4 * (cc + 1)));
    W.cstart = reinterpret_cast<int32_t*>(take(4 * (cc + 1)));
    W.shiftj = reinterpret_cast<double*>(take(8 * cc));
    W.colmean = reinterpret_cast<double*>(take(8 * kk));
    W.colvar = reinterpret_cast<double*>(take(8 * kk));
    W.partial = reinterpret_cast<double*>(take(8 * (nblk + cc) * kk));
    W.ipart = reinterpret_cast<double*>(take(8 * nblk));
    W.seed_m = reinterpret_cast<float*>(take(4 * nn));
    W.segt = reinterpret_cast<double*>(take(8 * nblk));
    W.bytes = off;
    return W;
}

static inline bool sizes_ok(int64_t n, int64_t C, int32_t k) { return n >= 1 && n <= INT32_MAX && C >= 1 && C <= n && k >= 1; }

// sum of one double per thread over a workgroup of 256, a fixed tree: t += t + 128, + 64, ... + 1.  s: 256 doubles of LDS.
__device__ __forceinline__ double block_sum_fixed(double v, double* s) {
    const int t = threadIdx.x;
    __syncthreads();   // (s may still be read from a previous call)
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    return s[0];
}

__global__ void kmeans_state_init_kernel(State* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        st->done = 0; st->n_iter = 0; st->converged = 0; st->changed = 0;
        st->tol_abs = 0.0; st->shift = 0.0; st->inertia = 0.0; st->reserved = 0.0;
    }
}

// ---- assignment ---------------------------------------------------------------------------------------
struct AssignParams {
    const float* X; int64_t n, ld;
    const float* B; int64_t nc, ld_c;
    int32_t k_int; int32_t first;     // first: the labels hold nothing to compare with
    int32_t* labels; float* dist; State* st;
};

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const AssignParams P) {
    __shared__ __attribute__((aligned(16))) float As[TK * TA];
    __shared__ __attribute__((aligned(16))) float Bs[TK * TB];
    __shared__ unsigned long long key_s[TA];
    if (P.st->done) return;   // the same value in every workgroup of the launch

    const int tid = threadIdx.x;
    const int tq = tid & 15, te = tid >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * TA;
    if (tid < TA) key_s[tid] = KEY_NONE;
    unsigned long long best[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};

    rowtile_stream<0>(P.X, P.n, P.ld, P.B, P.nc, P.ld_c, P.k_int, row0, (P.nc + TB - 1) / TB, As, Bs,
                      [&](int64_t tile, const float (&acc)[16]) __attribute__((always_inline)) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int64_t j = tile * TB + 4 * te + y;
                const float d = rowtile_distance<0>(acc[4 * x + y]);
                if (j < P.nc && d == d) best[x] = min(best[x], dist_key(d, j));   // (rows past n are clamped copies: not stored)
            }
    });
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 4; ++x)
        if (best[x] != KEY_NONE) atomicMin(&key_s[4 * tq + x], best[x]);   // LDS, integers: the minimum is order-free
    __syncthreads();
    int changed = 0;
    if (tid < TA && row0 + tid < P.n) {
        const unsigned long long key = key_s[tid];
        const int32_t lab = key == KEY_NONE ? -1 : (int32_t)(uint32_t)key;
        if (!P.first && P.labels[row0 + tid] != lab) changed = 1;
        P.labels[row0 + tid] = lab;
        P.dist[row0 + tid] = key == KEY_NONE ? INFINITY : key_dist(key);
    }
    if (__syncthreads_or(changed) && tid == 0) atomicOr(&P.st->changed, 1);
}

// ---- the stable counting sort of the rows by label -----------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t C,
                                                          int32_t* __restrict__ cnt, int32_t* __restrict__ rank, const State* st) {
    __shared__ int lab_s[CH];
    if (st->done) return;
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * CH + t;
    int32_t* row = cnt + (size_t)blockIdx.x * (size_t)C;
    for (int64_t j = t; j < C; j += CH) row[j] = 0;
    const int lab = i < n ? labels[i] : -1;
    lab_s[t] = lab;
    __syncthreads();   // (also orders the zeros above before the counts below: the stores have left the wave)
    if (lab >= 0) {
        int r = 0;
        bool last = true;
        for (int q = 0; q < CH; ++q) {
            const int o = lab_s[q];
            r += (o == lab && q < t);
            last = last && !(o == lab && q > t);
        }
        rank[i] = r;
        if (last) row[lab] = r + 1;
    }
}

__global__ __launch_bounds__(256) void kmeans_colscan_kernel(int32_t* __restrict__ cnt, int64_t nblk, int64_t C,
                                                             int32_t* __restrict__ count, const State* st) {
    if (st->done) return;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    int run = 0;
    for (int64_t b = 0; b < nblk; ++b) {
        const size_t at = (size_t)b * (size_t)C + (size_t)j;
        const int c = cnt[at];
        cnt[at] = run;
        run += c;
    }
    count[j] = run;
}

// one workgroup: start[j] = rows of the clusters below j, cstart[j] = their chunks; entry C holds the totals
__global__ __launch_bounds__(256) void kmeans_starts_kernel(const int32_t* __restrict__ count, int64_t C, int32_t* __restrict__ start,
                                                            int32_t* __restrict__ cstart, const State* st) {
    __shared__ int a_s[256], b_s[256];
    if (st->done) return;
    const int t = threadIdx.x;
    int carry_a = 0, carry_b = 0;
    for (int64_t j0 = 0; j0 < C; j0 += 256) {
        const int64_t j = j0 + t;
        const int c = j < C ? count[j] : 0;
        const int ch = (c + CH - 1) / CH;
        __syncthreads();
        a_s[t] = c; b_s[t] = ch;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {   // inclusive scan (integers: exact)
            const int va = t >= off ? a_s[t - off] : 0, vb = t >= off ? b_s[t - off] : 0;
            __syncthreads();
            a_s[t] += va; b_s[t] += vb;
            __syncthreads();
        }
        if (j < C) { start[j] = carry_a + a_s[t] - c; cstart[j] = carry_b + b_s[t] - ch; }
        carry_a += a_s[255]; carry_b += b_s[255];
    }
    if (t == 0) { start[C] = carry_a; cstart[C] = carry_b; }
}

__global__ __launch_bounds__(256) void kmeans_scatter_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ rank,
                                                             const int32_t* __restrict__ cnt, const int32_t* __restrict__ start,
                                                             int64_t n, int64_t C, int32_t* __restrict__ order, const State* st) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    if (i >= n) return;
    const int lab = labels[i];
    if (lab < 0) return;
    const int64_t pos = (int64_t)start[lab] + cnt[(size_t)blockIdx.x * (size_t)C + (size_t)lab] + rank[i];
    if (pos < n) order[pos] = (int32_t)i;   // (always: the positions of the labelled rows are a permutation of [0, start[C]))
}

// ---- chunk sums -------------------------------------------------------------------------------------------
// MODE 0: chunk g of the members (order[]) — the update; MODE 1: rows [256 g, 256 g + 256) — column sums; MODE 2: the same rows,
// (x - mean[col])^2.  A thread per column walks the chunk's rows one after the other.
template <int MODE>
__global__ __launch_bounds__(256) void kmeans_chunk_kernel(const float* __restrict__ X, int64_t n, int64_t ld, int32_t k_int, int64_t C,
                                                           const int32_t* __restrict__ order, const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ start, const int32_t* __restrict__ cstart,
                                                           const double* __restrict__ mean, double* __restrict__ partial,
                                                           const State* st) {
    __shared__ int row_s[CH];
    if (MODE == 0 && st->done) return;
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x;
    int m;
    if (MODE == 0) {
        if (g >= cstart[C]) return;
        int64_t lo = 0, hi = C;   // the cluster with cstart[j] <= g < cstart[j + 1]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (cstart[mid] <= g) lo = mid; else hi = mid;
        }
        const int64_t c = g - cstart[lo];
        const int64_t p0 = (int64_t)start[lo] + CH * c;
        m = (int)min((int64_t)CH, (int64_t)count[lo] - CH * c);
        row_s[t] = t < m ? order[p0 + t] : 0;
    } else {
        m = (int)min((int64_t)CH, n - CH * g);
        row_s[t] = t < m ? (int)(CH * g + t) : 0;
    }
    __syncthreads();
    for (int col = t; col < k_int; col += 256) {
        const double mu = MODE == 2 ? mean[col] : 0.0;
        double s = 0.0;
        for (int r = 0; r < m; ++r) {
            const double x = (double)X[(int64_t)row_s[r] * ld + col];
            if (MODE == 2) { const double d = x - mu; s += d * d; }
            else s += x;
        }
        partial[(size_t)g * (size_t)k_int + col] = s;
    }
}

// out[col] = (sum over the chunks, one after the other) / n
__global__ __launch_bounds__(256) void kmeans_colreduce_kernel(const double* __restrict__ partial, int64_t nchunks, int32_t k_int,
                                                               int64_t n, double* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= k_int) return;
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) s += partial[(size_t)c * (size_t)k_int + col];
    out[col] = s / (double)n;
}

__global__ void kmeans_tol_kernel(const double* __restrict__ colvar, int32_t k_int, double tol, State* st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int col = 0; col < k_int; ++col) s += colvar[col];
    st->tol_abs = tol * (s / (double)k_int);
}

// a workgroup per cluster: the new centre and the cluster's share of the shift
__global__ __launch_bounds__(256) void kmeans_centres_kernel(const double* __restrict__ partial, const int32_t* __restrict__ count,
                                                             const int32_t* __restrict__ cstart, int32_t k_int,
                                                             float* __restrict__ centres, int64_t ld_c, double* __restrict__ shiftj,
                                                             const State* st) {
    __shared__ double red_s[256];
    if (st->done) return;
    const int t = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int cn = count[j];
    double acc = 0.0;
    if (cn > 0) {   // an empty cluster keeps its centre
        const int64_t g0 = cstart[j], nch = cstart[j + 1] - g0;
        for (int col = t; col < k_int; col += 256) {
            double s = 0.0;
            for (int64_t c = 0; c < nch; ++c) s += partial[(size_t)(g0 + c) * (size_t)k_int + col];
            const float nw = (float)(s / (double)cn);
            const double d = (double)nw - (double)centres[j * ld_c + col];
            acc += d * d;
            centres[j * ld_c + col] = nw;
        }
    }
    const double total = block_sum_fixed(acc, red_s);
    if (t == 0) shiftj[j] = total;
}

__global__ __launch_bounds__(256) void kmeans_decide_kernel(const double* __restrict__ shiftj, int64_t C, State* st) {
    __shared__ double red_s[256];
    if (st->done) return;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < C; j += 256) s += shiftj[j];
    const double shift = block_sum_fixed(s, red_s);
    if (threadIdx.x == 0) {
        st->shift = shift;
        st->n_iter += 1;
        if (!st->changed || shift <= st->tol_abs) { st->done = 1; st->converged = 1; }
        st->changed = 0;
    }
}

// ---- inertia and info ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_inertia_kernel(const int32_t* __restrict__ labels, const float* __restrict__ dist,
                                                             int64_t n, double* __restrict__ ipart) {
    __shared__ double red_s[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < n && labels[i] >= 0) { const double d = (double)dist[i]; v = d * d; }
    const double total = block_sum_fixed(v, red_s);
    if (threadIdx.x == 0) ipart[blockIdx.x] = total;
}

// info: 4 x 8 bytes {double inertia, int64 n_iter, int64 converged, double tol_abs}
__global__ __launch_bounds__(256) void kmeans_info_kernel(const double* __restrict__ ipart, int64_t nblk, State* st, void* info) {
    __shared__ double red_s[256];
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += 256) s += ipart[b];
    const double inertia = block_sum_fixed(s, red_s);
    if (threadIdx.x == 0) {
        st->inertia = inertia;
        static_cast<double*>(info)[0] = inertia;
        static_cast<int64_t*>(info)[1] = st->n_iter;
        static_cast<int64_t*>(info)[2] = st->converged;
        static_cast<double*>(info)[3] = st->tol_abs;
    }
}

// ---- k-means++ seeding -----------------------------------------------------------------------------------
// m[i] = +inf; workgroup 0 takes row first_row as centre 0
__global__ __launch_bounds__(256) void seed_init_kernel(const float* __restrict__ X, int64_t n, int64_t ld, int32_t k_int,
                                                        int64_t first_row, float* __restrict__ m, float* __restrict__ centres,
                                                        int32_t* __restrict__ chosen) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) m[i] = INFINITY;
    if (blockIdx.x == 0) {
        for (int col = threadIdx.x; col < k_int; col += 256) centres[col] = X[first_row * ld + col];
        if (threadIdx.x == 0) chosen[0] = (int32_t)first_row;
    }
}

// m[i] = min(m[i], d(i, B row 0)): the tile stream with one row of B (its other 63 columns are clamped copies)
__global__ __launch_bounds__(256) void seed_dist_kernel(const float* __restrict__ X, int64_t n, int64_t ld, const float* __restrict__ B,
                                                        int32_t k_int, float* __restrict__ m) {
    __shared__ __attribute__((aligned(16))) float As[TK * TA];
    __shared__ __attribute__((aligned(16))) float Bs[TK * TB];
    const int tid = threadIdx.x;
    const int tq = tid & 15, te = tid >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * TA;
    rowtile_stream<0>(X, n, ld, B, 1, k_int, k_int, row0, 1, As, Bs,
                      [&](int64_t, const float (&acc)[16]) __attribute__((always_inline)) {
        if (te == 0) {   // B row 0 is y = 0 of the threads with te = 0; tq names the four rows: one thread per row
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int64_t i = row0 + 4 * tq + x;
                const float d = rowtile_distance<0>(acc[4 * x]);
                if (i < n && d < m[i]) m[i] = d;   // (a NaN is no candidate)
            }
        }
    });
}

__device__ __forceinline__ double seed_weight(float m) {
    const double d = (double)m;
    return m < INFINITY ? d * d : 0.0;   // a row without a finite distance is never drawn by weight
}

// a thread per segment of 256 consecutive rows: the segment's weights added one after the other
__global__ __launch_bounds__(256) void seed_segments_kernel(const float* __restrict__ m, int64_t n, double* __restrict__ segt) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s * CH >= n) return;
    const int64_t end = min(n, (s + 1) * CH);
    double run = 0.0;
    for (int64_t i = s * CH; i < end; ++i) run += seed_weight(m[i]);
    segt[s] = run;
}

// one workgroup; thread 0 walks the segments, then the rows of the segment the target falls in: S_i = P_s + r_i with P_s the
// segment totals added one after the other and r_i the running sum inside segment s — non-decreasing in i.  The pick is the
// first i with S_i > u S_n; floor(u n) when S_n == 0.  Then the workgroup copies the row.
__global__ __launch_bounds__(256) void seed_pick_kernel(const float* __restrict__ X, int64_t n, int64_t ld, int32_t k_int,
                                                        const float* __restrict__ m, const double* __restrict__ segt, int64_t nseg,
                                                        double u, float* __restrict__ centre, int32_t* __restrict__ chosen_c) {
    __shared__ long long pick_s;
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int64_t s = 0; s < nseg; ++s) total += segt[s];
        int64_t pick;
        if (!(total > 0.0)) {
            pick = (int64_t)(u * (double)n);
        } else {
            const double target = u * total;
            double P = 0.0;
            int64_t s = 0;
            for (; s < nseg - 1; ++s) {
                const double next = P + segt[s];
                if (next > target) break;
                P = next;
            }
            const int64_t end = min(n, (s + 1) * CH);
            pick = end - 1;
            double r = 0.0;
            for (int64_t i = s * CH; i < end; ++i) {
                r += seed_weight(m[i]);
                if (P + r > target) { pick = i; break; }
            }
        }
        pick = max((int64_t)0, min(pick, n - 1));
        pick_s = pick;
        *chosen_c = (int32_t)pick;
    }
    __syncthreads();
    const int64_t pick = pick_s;
    for (int col = threadIdx.x; col < k_int; col += 256) centre[col] = X[pick * ld + col];
}

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" size_t emg_rows_kmeans_ws_bytes(int64_t n, int64_t n_clusters, int32_t k_int) {
    if (!sizes_ok(n, n_clusters, k_int)) return 0;
    const size_t bytes = carve(nullptr, n, n_clusters, k_int).bytes;
    return bytes == SIZE_MAX ? 0 : bytes;
}

static int check_common(const char* who, const float* X, int64_t n, int64_t ld, int32_t k_int, const float* centres, int64_t ld_c,
                        int64_t n_clusters, void* ws, size_t ws_bytes, Workspace* W) {
    EMG_REQUIRE(sizes_ok(n, n_clusters, k_int) && ld >= k_int && ld_c >= k_int,
                "%s: bad sizes (1 <= n_clusters <= n <= INT32_MAX, k_int >= 1, ld >= k_int, ld_c >= k_int)", who);
    *W = carve(ws, n, n_clusters, k_int);
    EMG_REQUIRE(W->bytes != SIZE_MAX && ws_bytes >= W->bytes, "%s: the workspace holds %llu bytes, %llu are needed", who,
                (unsigned long long)ws_bytes, (unsigned long long)W->bytes);
    EMG_REQUIRE(ws && aligned16(ws), "%s: the workspace must be 16-byte aligned", who);
    EMG_REQUIRE(X && centres, "%s: null pointer", who);
    EMG_REQUIRE(cdiv(n, CH) + n_clusters < ((int64_t)1 << 31), "%s: grid too large", who);
    return EMG_OK;
}

extern "C" int emg_rows_kmeans(const float* X, int64_t n, int64_t ld, int32_t k_int, float* centres, int64_t ld_c,
                               int64_t n_clusters, int32_t max_iter, double tol, int32_t* labels, void* info, void* ws,
                               size_t ws_bytes, void* stream) {
    Workspace W;
    const int rc = check_common("emg_rows_kmeans", X, n, ld, k_int, centres, ld_c, n_clusters, ws, ws_bytes, &W);
    if (rc != EMG_OK) return rc;
    EMG_REQUIRE(max_iter >= 0, "emg_rows_kmeans: max_iter %d < 0", max_iter);
    EMG_REQUIRE(tol == tol && tol >= 0.0 && tol < INFINITY, "emg_rows_kmeans: tol must be a finite number >= 0");
    EMG_REQUIRE(labels, "emg_rows_kmeans: null pointer");
    EMG_REQUIRE(info && (reinterpret_cast<uintptr_t>(info) & 7u) == 0, "emg_rows_kmeans: info must be an 8-byte aligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t C = n_clusters, nblk = cdiv(n, CH);
    const dim3 wg(256);
    const unsigned g_rows = (unsigned)nblk, g_cols = (unsigned)cdiv(k_int, 256);

    hipLaunchKernelGGL(kmeans_state_init_kernel, dim3(1), dim3(64), 0, st, W.st);
    EMG_LAUNCH_CHECK();
    if (max_iter > 0) {   // tol_abs: two passes over the table, in f64
        hipLaunchKernelGGL(kmeans_chunk_kernel<1>, dim3(g_rows), wg, 0, st, X, n, ld, k_int, C, nullptr, nullptr, nullptr, nullptr,
                           nullptr, W.partial, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_colreduce_kernel, dim3(g_cols), wg, 0, st, W.partial, nblk, k_int, n, W.colmean);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_chunk_kernel<2>, dim3(g_rows), wg, 0, st, X, n, ld, k_int, C, nullptr, nullptr, nullptr, nullptr,
                           W.colmean, W.partial, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_colreduce_kernel, dim3(g_cols), wg, 0, st, W.partial, nblk, k_int, n, W.colvar);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_tol_kernel, dim3(1), dim3(64), 0, st, W.colvar, k_int, tol, W.st);
        EMG_LAUNCH_CHECK();
    }
    AssignParams A{};
    A.X = X; A.n = n; A.ld = ld; A.B = centres; A.nc = C; A.ld_c = ld_c; A.k_int = k_int; A.first = 1;
    A.labels = labels; A.dist = W.dist; A.st = W.st;
    const unsigned g_assign = (unsigned)cdiv(n, TA);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(g_assign), wg, 0, st, A);
    EMG_LAUNCH_CHECK();
    A.first = 0;
    for (int32_t it = 0; it < max_iter; ++it) {
        hipLaunchKernelGGL(kmeans_hist_kernel, dim3(g_rows), wg, 0, st, labels, n, C, W.cnt, W.rank, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_colscan_kernel, dim3((unsigned)cdiv(C, 256)), wg, 0, st, W.cnt, nblk, C, W.count, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_starts_kernel, dim3(1), wg, 0, st, W.count, C, W.start, W.cstart, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_scatter_kernel, dim3(g_rows), wg, 0, st, labels, W.rank, W.cnt, W.start, n, C, W.order, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_chunk_kernel<0>, dim3((unsigned)(nblk + C)), wg, 0, st, X, n, ld, k_int, C, W.order, W.count,
                           W.start, W.cstart, nullptr, W.partial, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_centres_kernel, dim3((unsigned)C), wg, 0, st, W.partial, W.count, W.cstart, k_int, centres, ld_c,
                           W.shiftj, W.st);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_assign_kernel, dim3(g_assign), wg, 0, st, A);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(kmeans_decide_kernel, dim3(1), wg, 0, st, W.shiftj, C, W.st);
        EMG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(g_rows), wg, 0, st, labels, W.dist, n, W.ipart);
    EMG_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_info_kernel, dim3(1), wg, 0, st, W.ipart, nblk, W.st, info);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_rows_kmeans_seed(const float* X, int64_t n, int64_t ld, int32_t k_int, int64_t n_clusters, int64_t first_row,
                                    const double* u, float* centres, int64_t ld_c, int32_t* chosen, void* ws, size_t ws_bytes,
                                    void* stream) {
    Workspace W;
    const int rc = check_common("emg_rows_kmeans_seed", X, n, ld, k_int, centres, ld_c, n_clusters, ws, ws_bytes, &W);
    if (rc != EMG_OK) return rc;
    EMG_REQUIRE(first_row >= 0 && first_row < n, "emg_rows_kmeans_seed: first_row %lld is outside [0, %lld)", (long long)first_row,
                (long long)n);
    EMG_REQUIRE(chosen && (n_clusters == 1 || u), "emg_rows_kmeans_seed: null pointer");
    for (int64_t c = 0; c + 1 < n_clusters; ++c)
        EMG_REQUIRE(u[c] >= 0.0 && u[c] < 1.0, "emg_rows_kmeans_seed: u[%lld] is outside [0, 1)", (long long)c);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nseg = cdiv(n, CH);
    const dim3 wg(256);
    hipLaunchKernelGGL(seed_init_kernel, dim3((unsigned)cdiv(n, 256)), wg, 0, st, X, n, ld, k_int, first_row, W.seed_m, centres, chosen);
    EMG_LAUNCH_CHECK();
    for (int64_t c = 1; c < n_clusters; ++c) {
        hipLaunchKernelGGL(seed_dist_kernel, dim3((unsigned)cdiv(n, TA)), wg, 0, st, X, n, ld, centres + (c - 1) * ld_c, k_int, W.seed_m);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(seed_segments_kernel, dim3((unsigned)cdiv(nseg, 256)), wg, 0, st, W.seed_m, n, W.segt);
        EMG_LAUNCH_CHECK();
        hipLaunchKernelGGL(seed_pick_kernel, dim3(1), wg, 0, st, X, n, ld, k_int, W.seed_m, W.segt, nseg, u[c - 1], centres + c * ld_c,
                           chosen + c);
        EMG_LAUNCH_CHECK();
    }
    return EMG_OK;
}
