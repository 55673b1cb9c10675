// emg_grid.hip — 1-vs-all counts of every query row against MANY thresholds (discover_facts' grid ranking).
//
// Extends "count the candidates that beat the positive" (EmbeddingModel.py:1856-1866 scored 1-vs-all, :2010-2033 compared;
// emg_rank.hip) from one comparison integer per query row to a list of them: the thresholds of a row are the comparison
// integers of the entities thr_ids[0..n_thr) scored against that row, and for each the kernel counts the entities outside the
// row's exclusion list whose comparison integer is greater / equal.  The scores are the canonical chain of emg_chain.hpp,
// bit-equal to emg_eval_scores_dense(precision 0); the [rows x |E|] matrix is never written.
//
// LAUNCH 1 (grid_thr_kernel, one workgroup per row): thread t scores entity thr_ids[t] against the row (chain_score), the row's
// thresholds are sorted and made distinct by counting (no sort network: n_thr <= 256), and the workspace receives the row's
// distinct ascending thresholds, their number and, for every t, the index of its threshold among them.  The counters are zeroed.
//
// LAUNCH 2 (grid_mfma_kernel / grid_transe_kernel): a workgroup takes GR query rows and one chunk of entity tiles.  LDS holds the
// rows' distinct thresholds and, per row, a histogram of 2 nd + 1 bins: bin 2j = "strictly between threshold j-1 and j", bin
// 2j + 1 = "equal to threshold j", bin 2 nd = "above every threshold".  Each finished score becomes its comparison integer, is
// dropped if its entity is in the row's exclusion list, is binary-searched in the row's thresholds and bumps one bin with an LDS
// atomic.  After the chunk a suffix sum over the bins (one wave per row) turns the histogram into gt / eq per distinct threshold,
// which go to the caller's (possibly repeated) thresholds with ONE global atomic per (row, threshold, counter) and workgroup.
#include <algorithm>

#include "emg_chain.hpp"

#pragma clang fp contract(off)

namespace emg {
namespace {

constexpr int GR = 32;    // query rows per workgroup: GR * TCAP * 12 bytes of thresholds and bins must fit LDS
constexpr int GN = 128;   // entities per tile
static_assert(EMG_GRID_THR_MAX == 256, "grid_thr_kernel: one thread per threshold; the kernels are instantiated for 64 / 128 / 256");

struct GridParams {
    const float* Q; int64_t ldq; int64_t n_rows;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    int32_t k_int; float scale; int32_t model; int32_t n_thr;
    const int32_t* thr_ids;
    const int64_t* excl_ptr; const int32_t* excl_idx;
    int32_t* nd;     // [n_rows]         number of distinct thresholds of the row
    int32_t* sthr;   // [n_rows][n_thr]  the distinct thresholds, ascending (the first nd[row] entries)
    int32_t* map;    // [n_rows][n_thr]  index of threshold t among them
    int32_t* cnt_gt; int32_t* cnt_eq;
    int64_t n_qb, n_cb, n_tiles; int32_t tiles_per_chunk;
};

__device__ __forceinline__ int cmp_int(float score) { return (int)__fmul_rn(score, 100000.0f); }   // as emg_rank.hip (EmbeddingModel.py:2010-2014)

// the model's final step on a finished chain (as chain_score's returns)
__device__ __forceinline__ float chain_final(int model, float scale, float acc) {
    if (model == EMG_HOLE) return __fmul_rn(acc, scale);
    if (model == EMG_TRANSE_L1) return -acc;
    if (model == EMG_TRANSE_L2) return -sqrtf(acc);
    if (model == EMG_TRANSE_P) return isinf(scale) ? -acc : -powf(acc, 1.0f / scale);
    return acc;
}

// ---------------------------------------------------------------------------------------------
// Launch 1: the thresholds of one row, sorted and distinct
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grid_thr_kernel(const GridParams P) {
    __shared__ int val[EMG_GRID_THR_MAX];
    __shared__ int srt[EMG_GRID_THR_MAX];
    const int64_t row = blockIdx.x;
    const int t = threadIdx.x, T = P.n_thr;
    int v = 0;
    if (t < T) {
        const int64_t e = min(max((int64_t)P.thr_ids[t], (int64_t)0), P.n_ent - 1);   // (an id outside the table reads a row inside it)
        v = cmp_int(chain_score(P.model, P.Q + row * P.ldq, P.ent + e * P.ld_ent, P.k_int, P.scale));
        val[t] = v;
        P.cnt_gt[row * T + t] = 0;
        P.cnt_eq[row * T + t] = 0;
    }
    __syncthreads();
    int pos = 0;
    if (t < T) {
        for (int u = 0; u < T; ++u) pos += (val[u] < v) || (val[u] == v && u < t);
        srt[pos] = v;
    }
    __syncthreads();
    if (t < T) {
        int d = 0;   // run heads in srt[1 .. pos]: the index of v among the distinct values
        for (int p = 1; p <= pos; ++p) d += srt[p] != srt[p - 1];
        P.map[row * T + t] = d;
        if (pos == 0 || srt[pos] != srt[pos - 1]) P.sthr[row * T + d] = v;
        if (pos == T - 1) P.nd[row] = d + 1;
    }
}

// ---------------------------------------------------------------------------------------------
// The histogram of a workgroup's GR rows
// ---------------------------------------------------------------------------------------------
template <int TCAP>
struct HistState {
    int64_t ex_lo[GR], ex_hi[GR];       // the row's range in excl_idx (empty: nothing excluded)
    int thr[GR][TCAP + 1];              // (+1: rows on different banks)
    unsigned hist[GR][2 * TCAP + 1];
    int nd[GR];                         // 0 for a row past n_rows
};

template <int TCAP>
__device__ __forceinline__ void hist_init(HistState<TCAP>& S, const GridParams& P, int64_t row0, int tid) {
    const int T = P.n_thr, NB = 2 * T + 1;
    if (tid < GR) {
        const int64_t row = row0 + tid;
        const bool in = row < P.n_rows;
        S.nd[tid] = in ? P.nd[row] : 0;
        S.ex_lo[tid] = (in && P.excl_ptr) ? P.excl_ptr[row] : 0;
        S.ex_hi[tid] = (in && P.excl_ptr) ? P.excl_ptr[row + 1] : 0;
    }
    for (int i = tid; i < GR * T; i += 256) {
        const int rl = i / T, t = i - rl * T;
        S.thr[rl][t] = row0 + rl < P.n_rows ? P.sthr[(row0 + rl) * T + t] : 0;   // (entries past nd[row] are never read)
    }
    for (int i = tid; i < GR * NB; i += 256) {
        const int rl = i / NB;
        S.hist[rl][i - rl * NB] = 0u;
    }
}

// one finished score of workgroup-local row rl and entity `col`
template <int TCAP>
__device__ __forceinline__ void hist_add(HistState<TCAP>& S, const GridParams& P, int64_t row0, int rl, int64_t col, float score) {
    if (col >= P.n_ent || row0 + rl >= P.n_rows) return;
    const int ci = cmp_int(score);
    int64_t lo = S.ex_lo[rl], hi = S.ex_hi[rl];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = P.excl_idx[mid];
        if (v == (int32_t)col) return;
        if (v < (int32_t)col) lo = mid + 1; else hi = mid;
    }
    const int n = S.nd[rl];
    int a = 0, b = n;
    while (a < b) {   // the first threshold that is not below ci
        const int mid = (a + b) >> 1;
        if (S.thr[rl][mid] < ci) a = mid + 1; else b = mid;
    }
    const int bin = 2 * a + (a < n && S.thr[rl][a] == ci);
    __hip_atomic_fetch_add(&S.hist[rl][bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// end of the chunk: bins -> "entities above bin b" (a suffix sum, wave w takes rows [8w, 8w + 8)), then one global add per
// (row, threshold, counter).  Called by all 256 threads.
template <int TCAP>
__device__ __forceinline__ void hist_finish(HistState<TCAP>& S, const GridParams& P, int64_t row0, int tid) {
    const int lane = tid & 63, wave = tid >> 6, T = P.n_thr;
    __syncthreads();
    for (int rl = wave * (GR / 4); rl < (wave + 1) * (GR / 4); ++rl) {
        const int nb = 2 * S.nd[rl] + 1;
        const int seg = (nb + 63) / 64;   // lane l owns bins [l seg, (l + 1) seg)
        const int b0 = min(lane * seg, nb), b1 = min(b0 + seg, nb);
        unsigned s = 0u;
        for (int b = b0; b < b1; ++b) s += S.hist[rl][b];
        unsigned tot = s;   // -> the sum over this lane and the lanes above it
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_down(tot, off, 64);
            if (lane + off < 64) tot += o;
        }
        unsigned run = tot - s;
        for (int b = b1 - 1; b >= b0; --b) {
            const unsigned h = S.hist[rl][b];
            S.hist[rl][b] = run;
            run += h;
        }
    }
    __syncthreads();
    for (int i = tid; i < GR * T; i += 256) {
        const int rl = i / T, t = i - rl * T;
        const int64_t row = row0 + rl;
        if (row >= P.n_rows) break;
        const int j = P.map[row * T + t];
        const unsigned gt = S.hist[rl][2 * j + 1], eq = S.hist[rl][2 * j] - gt;
        if (gt) atomicAdd(&P.cnt_gt[row * T + t], (int)gt);
        if (eq) atomicAdd(&P.cnt_eq[row * T + t], (int)eq);
    }
}

// XCD-aware decode (as the count kernels): the workgroups of one XCD walk the row tiles of the same entity chunk, which they
// then share in that XCD's L2
__device__ __forceinline__ bool decode_block(const GridParams& P, int64_t& qb, int64_t& cb) {
    const int64_t id = blockIdx.x;
    const int64_t xcd = id & 7, slot = id >> 3;
    qb = slot % P.n_qb;
    cb = xcd + 8 * (slot / P.n_qb);
    return cb < P.n_cb;
}

// ---------------------------------------------------------------------------------------------
// DistMult / ComplEx / HolE: the f32 MFMA main loop of count_mfma_pipe_kernel / topn_mfma_kernel — same operand order, same
// k-major LDS layout, next slice in flight under the MFMAs — on 32 x 128 tiles (wave w: the 32 x 32 block of entities
// [32 w, 32 w + 32)), with the histogram epilogue.  VEC: 16-byte row loads (16-byte-aligned rows, k_int % 4 == 0).
// ---------------------------------------------------------------------------------------------
constexpr int BK = 16, LDA = GR + 2, LDB = GN + 2;

template <int TCAP, bool VEC>
__global__ __launch_bounds__(256) void grid_mfma_kernel(const GridParams P) {
    __shared__ float As[BK * LDA];
    __shared__ float Bs[BK * LDB];
    __shared__ HistState<TCAP> S;

    int64_t qb, cb;
    if (!decode_block(P, qb, cb)) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = tid >> 2, kq = tid & 3;   // loader: entity rows lrow, lrow + 64 (query row lrow, threads < 128); floats [4kq, 4kq+4) of the slice
    const int l31 = lane & 31, lhi = lane >> 5;
    const int64_t row0 = qb * GR;
    const bool a_ld = tid < 4 * GR;

    hist_init<TCAP>(S, P, row0, tid);

    const float* arow = P.Q + min(row0 + (lrow & (GR - 1)), P.n_rows - 1) * P.ldq + 4 * kq;
    const float* brow[2];
    auto point_b = [&](int64_t tile) {
#pragma unroll
        for (int r = 0; r < 2; ++r) brow[r] = P.ent + min(tile * GN + lrow + 64 * r, P.n_ent - 1) * P.ld_ent + 4 * kq;
    };
    f32x4 av, bv[2];
    auto fetch = [&](int k0) {
        const int kb = k0 + 4 * kq;
        if constexpr (VEC) {   // k_int % 4 == 0: a 4-float piece is either whole or past the end
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            const bool in = kb < P.k_int;
            av = in ? *reinterpret_cast<const f32x4*>(arow + k0) : zero4;
#pragma unroll
            for (int r = 0; r < 2; ++r) bv[r] = in ? *reinterpret_cast<const f32x4*>(brow[r] + k0) : zero4;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool in = kb + c < P.k_int;
                av[c] = in ? arow[k0 + c] : 0.f;
#pragma unroll
                for (int r = 0; r < 2; ++r) bv[r][c] = in ? brow[r][k0 + c] : 0.f;
            }
        }
    };

    const int64_t tile0 = cb * P.tiles_per_chunk;
    const int64_t tile1 = min(tile0 + (int64_t)P.tiles_per_chunk, P.n_tiles);
    point_b(tile0);
    fetch(0);
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        float16v acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;

        for (int k0 = 0; k0 < P.k_int; k0 += BK) {
            __syncthreads();   // previous slice's LDS reads done (first slice: the histogram is initialised)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a_ld) As[(4 * kq + c) * LDA + lrow] = av[c];
#pragma unroll
                for (int r = 0; r < 2; ++r) Bs[(4 * kq + c) * LDB + lrow + 64 * r] = bv[r][c];
            }
            __syncthreads();
            // next slice (or the next tile's first one) flies while this one is multiplied
            if (k0 + BK < P.k_int) fetch(k0 + BK);
            else if (tile + 1 < tile1) { point_b(tile + 1); fetch(0); }
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk) {
                const int k = 2 * kk + lhi;   // A[i][k=lane>>5], B[k=lane>>5][j]
                const float a = As[k * LDA + l31];
                const float b = Bs[k * LDB + wave * 32 + l31];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
        // D[row][col]: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
        const int64_t col = tile * GN + wave * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            hist_add<TCAP>(S, P, row0, (r & 3) + 8 * (r >> 2) + 4 * lhi, col, chain_final(P.model, P.scale, acc[r]));
    }
    hist_finish<TCAP>(S, P, row0, tid);
}

// ---------------------------------------------------------------------------------------------
// TransE (L1, L2, any order): the VALU chain main loop of topn_transe_kernel — 4 x 4 chains per thread, k tiles staged in LDS —
// on 32 queries x 128 entities per workgroup, with the histogram epilogue.  KIND 1 / 2: chain_step; 3: the powf / max step of
// EMG_TRANSE_P.  The k loop stops at k_int, so every chain takes exactly chain_score's steps.
// ---------------------------------------------------------------------------------------------
constexpr int TK = 32;

template <int TCAP, int KIND>
__global__ __launch_bounds__(256) void grid_transe_kernel(const GridParams P) {
    __shared__ __attribute__((aligned(16))) float Qs[TK * GR];
    __shared__ __attribute__((aligned(16))) float Es[TK * GN];
    __shared__ HistState<TCAP> S;

    int64_t qb, cb;
    if (!decode_block(P, qb, cb)) return;

    const int tid = threadIdx.x;
    const int tq = tid & 7, te = tid >> 3;         // chains: query rows [4tq, 4tq+4) x entities [4te, 4te+4)
    const int qrow = tid & 31, qs = tid >> 5;      // loader: query row qrow, 4-float slot qs of the k tile
    const int erow = tid & 127, es = tid >> 7;     //         entity row erow, slots es, es + 2, es + 4, es + 6
    const int64_t row0 = qb * GR;

    hist_init<TCAP>(S, P, row0, tid);

    const float* qptr = P.Q + min(row0 + qrow, P.n_rows - 1) * P.ldq;
    const bool ord_inf = isinf(P.scale);

    const int64_t tile0 = cb * P.tiles_per_chunk;
    const int64_t tile1 = min(tile0 + (int64_t)P.tiles_per_chunk, P.n_tiles);
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const float* eptr = P.ent + min(tile * GN + erow, P.n_ent - 1) * P.ld_ent;
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < P.k_int; k0 += TK) {
            float qv[4], ev[4][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) qv[c] = k0 + 4 * qs + c < P.k_int ? qptr[k0 + 4 * qs + c] : 0.f;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int kb = k0 + 4 * (es + 2 * h);
#pragma unroll
                for (int c = 0; c < 4; ++c) ev[h][c] = kb + c < P.k_int ? eptr[kb + c] : 0.f;
            }
            __syncthreads();   // previous k tile's LDS reads done (first one: the histogram is initialised)
#pragma unroll
            for (int c = 0; c < 4; ++c) Qs[(4 * qs + c) * GR + qrow] = qv[c];
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int c = 0; c < 4; ++c) Es[(4 * (es + 2 * h) + c) * GN + erow] = ev[h][c];
            __syncthreads();
            const int kn = min(TK, P.k_int - k0);
            for (int k = 0; k < kn; ++k) {
                const float4 q4 = *reinterpret_cast<const float4*>(&Qs[k * GR + 4 * tq]);
                const float4 e4 = *reinterpret_cast<const float4*>(&Es[k * GN + 4 * te]);
                const float q[4] = {q4.x, q4.y, q4.z, q4.w};
                const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if constexpr (KIND == 3) {
                            const float d = fabsf(__fsub_rn(q[a], e[b]));
                            acc[4 * a + b] = ord_inf ? fmaxf(acc[4 * a + b], d) : __fadd_rn(acc[4 * a + b], powf(d, P.scale));
                        } else {
                            acc[4 * a + b] = chain_step<KIND>(q[a], e[b], acc[4 * a + b]);
                        }
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            hist_add<TCAP>(S, P, row0, 4 * tq + (r >> 2), tile * GN + 4 * te + (r & 3), chain_final(P.model, P.scale, acc[r]));
    }
    hist_finish<TCAP>(S, P, row0, tid);
}

// bytes of nd, sthr and map; -1: the product does not fit int64
int64_t grid_ws_bytes(int64_t n_rows, int32_t n_thr) {
    int64_t b;
    if (__builtin_mul_overflow(n_rows, (2 * (int64_t)n_thr + 1) * (int64_t)sizeof(int32_t), &b)) return -1;
    return b;
}

template <int TCAP>
void (*grid_kernel(int model, bool vec))(const GridParams) {
    switch (model) {
        case EMG_TRANSE_L1: return grid_transe_kernel<TCAP, 1>;
        case EMG_TRANSE_L2: return grid_transe_kernel<TCAP, 2>;
        case EMG_TRANSE_P: return grid_transe_kernel<TCAP, 3>;
        default: return vec ? grid_mfma_kernel<TCAP, true> : grid_mfma_kernel<TCAP, false>;
    }
}

constexpr int64_t GRID_TARGET_BLOCKS = 1024;   // the entity range is cut so that about this many workgroups share a call
constexpr int64_t GRID_MIN_TILES = 4;          // ... but a workgroup's histogram set-up and flush are spread over at least 4 tiles

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" int64_t emg_eval_grid_ws_bytes(int64_t n_rows, int32_t n_thr) {
    EMG_REQUIRE(n_rows >= 0, "emg_eval_grid_ws_bytes: bad sizes");
    EMG_REQUIRE(n_thr >= 1 && n_thr <= EMG_GRID_THR_MAX, "emg_eval_grid_ws_bytes: n_thr %d outside [1, %d]", (int)n_thr, EMG_GRID_THR_MAX);
    const int64_t b = grid_ws_bytes(n_rows, n_thr);
    EMG_REQUIRE(b >= 0, "emg_eval_grid_ws_bytes: the workspace size does not fit 64 bits");
    return b;
}

extern "C" int emg_eval_grid_count(int model, const float* Q, int64_t ldq, int64_t n_rows, const float* ent, int64_t n_ent,
                                   int64_t ld_ent, int32_t k_int, float scale, const int32_t* thr_ids, int32_t n_thr,
                                   const int64_t* excl_ptr, const int32_t* excl_idx, void* ws, int64_t ws_bytes, int32_t* cnt_gt,
                                   int32_t* cnt_eq, void* stream) {
    model = chain_model(model);
    EMG_REQUIRE(model >= 0 && model <= EMG_TRANSE_P, "emg_eval_grid_count: unknown model id %d", model);
    EMG_REQUIRE(n_thr >= 1 && n_thr <= EMG_GRID_THR_MAX, "emg_eval_grid_count: n_thr %d outside [1, %d]", (int)n_thr, EMG_GRID_THR_MAX);
    EMG_REQUIRE(n_rows >= 0 && n_ent >= 1 && n_ent <= INT32_MAX && k_int > 0 && ldq >= k_int && ld_ent >= k_int && ws_bytes >= 0,
                "emg_eval_grid_count: bad sizes");
    EMG_REQUIRE(model != EMG_TRANSE_P || scale > 0.f, "EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive");
    if (n_rows == 0) return EMG_OK;
    EMG_REQUIRE(Q && ent && thr_ids && cnt_gt && cnt_eq, "emg_eval_grid_count: null pointer");
    const int64_t need = grid_ws_bytes(n_rows, n_thr);
    EMG_REQUIRE(need >= 0 && need <= ws_bytes && ws, "emg_eval_grid_count: workspace of %lld bytes, emg_eval_grid_ws_bytes asks for %lld",
                (long long)ws_bytes, (long long)need);
    EMG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "emg_eval_grid_count: the workspace must be 4-byte aligned");
    EMG_REQUIRE(n_rows < ((int64_t)1 << 31), "emg_eval_grid_count: grid too large");
    hipStream_t st = (hipStream_t)stream;
    GridParams P{};
    P.Q = Q; P.ldq = ldq; P.n_rows = n_rows; P.ent = ent; P.n_ent = n_ent; P.ld_ent = ld_ent;
    P.k_int = k_int; P.scale = scale; P.model = model; P.n_thr = n_thr; P.thr_ids = thr_ids;
    P.excl_ptr = excl_ptr; P.excl_idx = excl_idx; P.cnt_gt = cnt_gt; P.cnt_eq = cnt_eq;
    P.nd = static_cast<int32_t*>(ws);
    P.sthr = P.nd + n_rows;
    P.map = P.sthr + n_rows * n_thr;
    P.n_qb = cdiv(n_rows, GR);
    P.n_tiles = cdiv(n_ent, GN);
    P.tiles_per_chunk = (int32_t)std::min(P.n_tiles, std::max(GRID_MIN_TILES, cdiv(P.n_tiles * P.n_qb, GRID_TARGET_BLOCKS)));
    P.n_cb = cdiv(P.n_tiles, P.tiles_per_chunk);
    const int64_t blocks = 8 * P.n_qb * cdiv(P.n_cb, 8);
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_eval_grid_count: grid too large");

    hipLaunchKernelGGL(grid_thr_kernel, dim3((unsigned)n_rows), dim3(256), 0, st, P);
    EMG_LAUNCH_CHECK();
    const bool vec = (ldq % 4 == 0) && (ld_ent % 4 == 0) && aligned16(Q) && aligned16(ent) && k_int % 4 == 0;
    void (*fn)(const GridParams) = n_thr <= 64 ? grid_kernel<64>(model, vec) : (n_thr <= 128 ? grid_kernel<128>(model, vec) : grid_kernel<256>(model, vec));
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), 0, st, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
