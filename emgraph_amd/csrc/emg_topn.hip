// emg_topn.hip — top-N completions: exact 1-vs-all scoring with the selection fused into the epilogue.
//
// Extends the 1-vs-all scoring of EmbeddingModel.py:1856-1866 (every entity scored against a query) from "count the
// candidates that beat the positive" (emg_rank.hip) to "keep the best N".  The scores are the canonical chain of
// emg_chain.hpp, bit-equal to emg_eval_scores_dense(precision 0); the [rows x |E|] matrix is never written.
//
// TOTAL ORDER (a 64-bit key per (score, id), order_key): higher score first, -0 == +0, NaN below every number and equal
// among themselves, equal scores by ascending GLOBAL entity id.  An entry is (score bits << 32) | id; padding is
// (-inf, -1) and sorts below everything.
//
// PHASE 1 (topn_mfma_kernel / topn_transe_kernel): a workgroup takes one tile of query rows and one chunk of candidate
// tiles.  Per row, LDS holds tau (the row's current N-th best, as a float for the one compare the hot epilogue makes per
// score, and as a key for the exact decision) and a SEL_B-entry append buffer; the row's sorted list lives in the caller's
// workspace slot of (row, chunk), which stays in L2.  A score that is not below tau takes the rare path: exact key compare,
// binary search in the row's ascending exclusion list, append.  A full buffer is merged into the list by one wave
// (merge_into: every element finds its place by counting, no sort network) and tau is raised; the lanes whose append found
// no room try again.  PHASE 2 (topn_merge_kernel): one wave per row merges the chunk lists, which are sorted, so a chunk is
// left at its first entry that no longer beats tau.
#include "emg_chain.hpp"

#pragma clang fp contract(off)

namespace emg {
namespace {

constexpr int SEL_B = 32;                             // append buffer entries per row (one per lane of half a wave)
constexpr uint64_t SEL_PAD = 0xff800000ffffffffull;   // (-inf, id -1)
constexpr int64_t TOPN_CHUNK = 16384;                 // candidates per chunk when the caller leaves the choice
constexpr int TOPN_TILE = 256;                        // chunks are whole tiles of either kernel (128 and 64 candidates)
static_assert(EMG_TOPN_MAX <= 128, "merge_into holds a list in two registers per lane");

struct TopnParams {
    const float* Q; int64_t ldq; int64_t n_rows;
    const float* ent; int64_t n_cand; int64_t ld_ent; const int32_t* cand; int64_t ent_offset;
    int32_t k_int; float scale; int32_t model; int32_t top_n;
    const int64_t* excl_ptr; const int32_t* excl_idx;
    uint64_t* lists;   // [n_rows][n_cb][top_n], each sorted best first, padded with SEL_PAD
    int64_t n_qb, n_cb, n_tiles; int32_t tiles_per_chunk;
};

// larger key = earlier in the total order; 0 = padding
__device__ __forceinline__ uint64_t order_key(uint64_t e) {
    const uint32_t id = (uint32_t)e, u = (uint32_t)(e >> 32);
    if (id == 0xffffffffu) return 0;
    uint32_t k;
    if ((u & 0x7fffffffu) > 0x7f800000u) k = 0u;              // NaN: below -inf (whose key is 0x007fffff)
    else if (u == 0x80000000u) k = 0x80000000u;               // -0 is +0
    else k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)k << 32) | (uint32_t)~id;               // ids are < 2^31: the low word is never 0
}

// the model's final step on a finished chain (as chain_score's returns)
__device__ __forceinline__ float chain_final(int model, float scale, float acc) {
    if (model == EMG_HOLE) return __fmul_rn(acc, scale);
    if (model == EMG_TRANSE_L1 || model == EMG_ROTATE) return -acc;
    if (model == EMG_TRANSE_L2) return -sqrtf(acc);
    if (model == EMG_TRANSE_P) return isinf(scale) ? -acc : -powf(acc, 1.0f / scale);
    return acc;
}

__device__ __forceinline__ void wave_sync() {   // this wave's earlier LDS / global writes are visible to its later reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One wave merges c <= SEL_B distinct unsorted entries buf[0..c) (none of them padding) into the sorted list[0..L), L <= N <= 128,
// keeping the N best.  Lane i holds list entries i and i + 64, lane j < c buffer entry j; an entry's new position is its own
// index plus the number of entries of the other array ahead of it (the buffer's: also those of its own array), counted in one
// loop over the buffer.  Returns the new length; writes tau when the list is full.  LIST_GLOBAL: the list is in global memory
// and was written by this workgroup (loads bypass the vector L1).
template <bool LIST_GLOBAL>
__device__ __forceinline__ int merge_into(uint64_t* list, int L, int N, const uint64_t* buf, int c, int lane, float* tau_f,
                                          uint64_t* tau_key) {
    uint64_t l[2], lk[2];
    int sh[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        l[h] = SEL_PAD;
        if (i < L) {
            if constexpr (LIST_GLOBAL) l[h] = __hip_atomic_load(list + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else l[h] = list[i];
        }
        lk[h] = order_key(l[h]);   // 0 past the list's end: behind every buffer entry
    }
    const uint64_t mine = lane < c ? buf[lane] : SEL_PAD;
    const uint64_t mk = order_key(mine);
    int rank = 0;
    for (int j = 0; j < c; ++j) {
        const uint64_t bk = order_key(buf[j]);
        const bool g0 = lk[0] >= bk, g1 = lk[1] >= bk;   // the list entry stays ahead of buffer entry j
        const int ahead = __popcll(__ballot(g0)) + __popcll(__ballot(g1));
        if (lane == j) rank += ahead;
        sh[0] += !g0; sh[1] += !g1;
        rank += (bk > mk) || (bk == mk && j < lane);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h, p = i + sh[h];
        if (i < L && p < N) {
            list[p] = l[h];
            if (p == N - 1) { *tau_f = __uint_as_float((uint32_t)(l[h] >> 32)); *tau_key = lk[h]; }
        }
    }
    if (lane < c && rank < N) {
        list[rank] = mine;
        if (rank == N - 1) { *tau_f = __uint_as_float((uint32_t)(mine >> 32)); *tau_key = mk; }
    }
    return min(L + c, N);
}

// element r of a register vector, r not known at compile time (a select chain: indexing would put the vector in scratch)
__device__ __forceinline__ float pick16(const float16v& v, int r) {
    float x = v[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) x = r == i ? v[i] : x;
    return x;
}

template <int ROWS>
struct SelState {
    uint64_t buf[ROWS][SEL_B];
    uint64_t tau_key[ROWS];   // key of the list's N-th entry; 0 while the list is short (everything enters)
    float tau_f[ROWS];        // its score; -inf while the list is short.  A score below it cannot enter.
    int cnt[ROWS];            // appends asked for since the row's last merge (those past SEL_B found no room)
    int len[ROWS];
    int work;
};

template <int ROWS>
__device__ __forceinline__ void sel_init(SelState<ROWS>& S, int tid) {
    if (tid < ROWS) { S.tau_key[tid] = 0; S.tau_f[tid] = -INFINITY; S.cnt[tid] = 0; S.len[tid] = 0; }
    if (tid == 0) S.work = 0;
}

__device__ __forceinline__ bool excluded(const TopnParams& P, int64_t qr, int32_t id) {
    if (!P.excl_ptr) return false;
    int64_t lo = P.excl_ptr[qr], hi = P.excl_ptr[qr + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = P.excl_idx[mid];
        if (v == id) return true;
        if (v < id) lo = mid + 1; else hi = mid;
    }
    return false;
}

// wave `wave` of a 4-wave workgroup merges the buffers of its ROWS / 4 rows that hold at least `min_cnt` appends
template <int ROWS>
__device__ __forceinline__ void sel_merge_rows(SelState<ROWS>& S, const TopnParams& P, int64_t row0, int64_t cb, int wave, int lane,
                                               int min_cnt) {
    for (int rl = wave * (ROWS / 4); rl < (wave + 1) * (ROWS / 4); ++rl) {
        const int n = S.cnt[rl];
        if (n < min_cnt || n == 0) continue;   // (rows past n_rows never append)
        uint64_t* list = P.lists + ((row0 + rl) * P.n_cb + cb) * P.top_n;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the list's earlier stores (this wave's own) are what the loads see
        const int L = merge_into<true>(list, S.len[rl], P.top_n, S.buf[rl], min(n, SEL_B), lane, &S.tau_f[rl], &S.tau_key[rl]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        wave_sync();
        if (lane == 0) { S.len[rl] = L; S.cnt[rl] = 0; }
    }
}

// The selection epilogue of one candidate tile.  Each thread holds NG groups of 16 finished chains; geo(g, r, rl, col) names the
// workgroup-local row and the candidate (index into the call's candidates) of chain r of group g.  Called by all 256 threads.
template <int ROWS, int NG, class Geo>
__device__ __forceinline__ void select_tile(SelState<ROWS>& S, const TopnParams& P, int64_t row0, int64_t cb, const float16v (&acc)[NG],
                                            Geo geo) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned pend[NG];
    unsigned any = 0u;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        pend[g] = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int rl; int64_t col;
            geo(g, r, rl, col);
            const float v = chain_final(P.model, P.scale, acc[g][r]);
            const bool in = col < P.n_cand && row0 + rl < P.n_rows;
            pend[g] |= (unsigned)(in && !(v < S.tau_f[rl])) << r;   // the one compare per score (a NaN goes on: it may fill a short list)
        }
        any |= pend[g];
    }
    if (any) S.work = 1;
    __syncthreads();
    while (S.work) {   // workgroup-uniform
        __syncthreads();
        if (tid == 0) S.work = 0;
        __syncthreads();
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            unsigned m = pend[g];
            while (m) {
                const int r = __ffs(m) - 1;
                m &= m - 1u;
                int rl; int64_t col;
                geo(g, r, rl, col);
                const float v = chain_final(P.model, P.scale, pick16(acc[g], r));
                const int32_t id = P.cand ? P.cand[col] : (int32_t)(P.ent_offset + col);
                const uint64_t e = ((uint64_t)__float_as_uint(v) << 32) | (uint32_t)id;
                bool done = true;
                if (order_key(e) > S.tau_key[rl] && !excluded(P, row0 + rl, id)) {
                    const int slot = atomicAdd(&S.cnt[rl], 1);
                    if (slot < SEL_B) S.buf[rl][slot] = e;
                    else { done = false; S.work = 1; }   // no room: again after the row's merge
                }
                if (done) pend[g] &= ~(1u << r);
            }
        }
        __syncthreads();
        if (S.work) sel_merge_rows<ROWS>(S, P, row0, cb, wave, lane, SEL_B);
        __syncthreads();
    }
}

// end of the chunk: the rows' last appends go into their lists, short lists are padded
template <int ROWS>
__device__ __forceinline__ void select_finish(SelState<ROWS>& S, const TopnParams& P, int64_t row0, int64_t cb) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();
    sel_merge_rows<ROWS>(S, P, row0, cb, wave, lane, 1);
    for (int rl = wave * (ROWS / 4); rl < (wave + 1) * (ROWS / 4); ++rl) {
        if (row0 + rl >= P.n_rows) break;
        uint64_t* list = P.lists + ((row0 + rl) * P.n_cb + cb) * P.top_n;
        for (int i = S.len[rl] + lane; i < P.top_n; i += 64) list[i] = SEL_PAD;
    }
}

// ---------------------------------------------------------------------------------------------
// DistMult / ComplEx / HolE: the f32 MFMA main loop of count_mfma_pipe_kernel (emg_rank.hip) — same operand order, same
// k-major LDS layout, next slice in flight under the MFMAs — with the selection epilogue.  VEC: 16-byte row loads
// (16-byte-aligned rows, k_int % 4 == 0); otherwise scalar loads, rows of any alignment and width.
// ---------------------------------------------------------------------------------------------
constexpr int BM = 128, BK = 16, LDK = 130, NTB = 2;   // 128 x 128 tiles: the 128 x 256 form of the count kernel leaves the selection no registers
constexpr int BNW = 2 * 32 * NTB, LDB = BNW + 2, NBR = BNW / 64;
static_assert(TOPN_TILE % BNW == 0, "chunks are whole tiles");

template <bool VEC>
__global__ __launch_bounds__(256, 2) void topn_mfma_kernel(const TopnParams P) {
    __shared__ float As[BK * LDK];
    __shared__ float Bs[BK * LDB];
    __shared__ SelState<BM> S;

    // XCD-aware decode (as the count kernels): the blocks of one XCD walk the query tiles of the same chunk
    const int64_t id = blockIdx.x;
    const int64_t xcd = id & 7, slot = id >> 3;
    const int64_t qb = slot % P.n_qb;
    const int64_t cb = xcd + 8 * (slot / P.n_qb);
    if (cb >= P.n_cb) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int lrow = tid >> 2, kq = tid & 3;  // loader: rows lrow, lrow+64 ; floats [4kq,4kq+4) of the 16-wide slice
    const int l31 = lane & 31, lhi = lane >> 5;
    const int64_t row0 = qb * BM;

    sel_init<BM>(S, tid);

    const float* arow[2];
    const float* brow[NBR];
#pragma unroll
    for (int r = 0; r < 2; ++r) arow[r] = P.Q + min(row0 + lrow + 64 * r, P.n_rows - 1) * P.ldq + 4 * kq;
    auto point_b = [&](int64_t tile) {
#pragma unroll
        for (int r = 0; r < NBR; ++r) {
            const int64_t el = min(tile * BNW + lrow + 64 * r, P.n_cand - 1);
            brow[r] = P.ent + (P.cand ? (int64_t)P.cand[el] : el) * P.ld_ent + 4 * kq;
        }
    };
    f32x4 av[2], bv[NBR];
    auto fetch = [&](int k0) {
        const int kb = k0 + 4 * kq;
        if constexpr (VEC) {   // k_int % 4 == 0: a 4-float piece is either whole or past the end
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            const bool in = kb < P.k_int;
#pragma unroll
            for (int r = 0; r < 2; ++r) av[r] = in ? *reinterpret_cast<const f32x4*>(arow[r] + k0) : zero4;
#pragma unroll
            for (int r = 0; r < NBR; ++r) bv[r] = in ? *reinterpret_cast<const f32x4*>(brow[r] + k0) : zero4;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool in = kb + c < P.k_int;
#pragma unroll
                for (int r = 0; r < 2; ++r) av[r][c] = in ? arow[r][k0 + c] : 0.f;
#pragma unroll
                for (int r = 0; r < NBR; ++r) bv[r][c] = in ? brow[r][k0 + c] : 0.f;
            }
        }
    };

    const int64_t tile0 = cb * P.tiles_per_chunk;
    const int64_t tile1 = min(tile0 + (int64_t)P.tiles_per_chunk, P.n_tiles);
    point_b(tile0);
    fetch(0);
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        float16v acc[2 * NTB];
#pragma unroll
        for (int g = 0; g < 2 * NTB; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;

        for (int k0 = 0; k0 < P.k_int; k0 += BK) {
            __syncthreads();  // previous slice's LDS reads done (first slice: the selection state is initialised / merged)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int r = 0; r < 2; ++r) As[(4 * kq + c) * LDK + lrow + 64 * r] = av[r][c];
#pragma unroll
                for (int r = 0; r < NBR; ++r) Bs[(4 * kq + c) * LDB + lrow + 64 * r] = bv[r][c];
            }
            __syncthreads();
            // next slice (or the next tile's first one) flies while this one is multiplied
            if (k0 + BK < P.k_int) fetch(k0 + BK);
            else if (tile + 1 < tile1) { point_b(tile + 1); fetch(0); }
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk) {
                const int k = 2 * kk + lhi;  // A[i][k=lane>>5], B[k=lane>>5][j]
                float a[2], b[NTB];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = As[k * LDK + wr * 64 + t * 32 + l31];
#pragma unroll
                for (int t = 0; t < NTB; ++t) b[t] = Bs[k * LDB + wc * (32 * NTB) + t * 32 + l31];
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb)
                        acc[ta * NTB + tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ta], b[tb], acc[ta * NTB + tb], 0, 0, 0);
            }
        }
        // D[row][col] of group g = ta * NTB + tb: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
        select_tile<BM, 2 * NTB>(S, P, row0, cb, acc, [&](int g, int r, int& rl, int64_t& col) {
            rl = wr * 64 + (g / NTB) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            col = tile * BNW + wc * (32 * NTB) + (g % NTB) * 32 + l31;
        });
    }
    select_finish<BM>(S, P, row0, cb);
}

// ---------------------------------------------------------------------------------------------
// TransE (L1, L2, any order): a VALU chain main loop, 64 queries x 64 candidates per workgroup, 4 x 4 per thread, k tiles
// staged in LDS (the shape of count_transe_kernel), and the same selection epilogue.  KIND 1 / 2: chain_step; 3: the
// powf / max step of EMG_TRANSE_P.  The k loop stops at k_int, so every chain takes exactly chain_score's steps.
// ---------------------------------------------------------------------------------------------
constexpr int TQ = 64, TE = 64, TK = 32;

template <int KIND>
__global__ __launch_bounds__(256) void topn_transe_kernel(const TopnParams P) {
    __shared__ __attribute__((aligned(16))) float Qs[TK * TQ];
    __shared__ __attribute__((aligned(16))) float Es[TK * TE];
    __shared__ SelState<TQ> S;

    const int64_t id = blockIdx.x;
    const int64_t xcd = id & 7, slot = id >> 3;
    const int64_t qb = slot % P.n_qb;
    const int64_t cb = xcd + 8 * (slot / P.n_qb);
    if (cb >= P.n_cb) return;

    const int tid = threadIdx.x;
    const int tq = tid & 15, te = tid >> 4;
    const int lrow = tid & 63, lkq = tid >> 6;  // loader: row lrow, 4-float slots lkq and lkq+4 of the k-tile
    const int64_t row0 = qb * TQ;

    sel_init<TQ>(S, tid);

    const float* qptr = P.Q + min(row0 + lrow, P.n_rows - 1) * P.ldq;
    const bool ord_inf = isinf(P.scale);

    const int64_t tile0 = cb * P.tiles_per_chunk;
    const int64_t tile1 = min(tile0 + (int64_t)P.tiles_per_chunk, P.n_tiles);
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t el = min(tile * TE + lrow, P.n_cand - 1);
        const float* eptr = P.ent + (P.cand ? (int64_t)P.cand[el] : el) * P.ld_ent;
        float16v acc[1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
        for (int k0 = 0; k0 < P.k_int; k0 += TK) {
            float qv[2][4], ev[2][4];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kb = k0 + 4 * (lkq + 4 * h);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    qv[h][c] = kb + c < P.k_int ? qptr[kb + c] : 0.f;
                    ev[h][c] = kb + c < P.k_int ? eptr[kb + c] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int kl = 4 * (lkq + 4 * h) + c;
                    Qs[kl * TQ + lrow] = qv[h][c];
                    Es[kl * TE + lrow] = ev[h][c];
                }
            __syncthreads();
            const int kn = min(TK, P.k_int - k0);
            for (int k = 0; k < kn; ++k) {
                const float4 q4 = *reinterpret_cast<const float4*>(&Qs[k * TQ + 4 * tq]);
                const float4 e4 = *reinterpret_cast<const float4*>(&Es[k * TE + 4 * te]);
                const float q[4] = {q4.x, q4.y, q4.z, q4.w};
                const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if constexpr (KIND == 3) {
                            const float d = fabsf(__fsub_rn(q[a], e[b]));
                            acc[0][4 * a + b] = ord_inf ? fmaxf(acc[0][4 * a + b], d) : __fadd_rn(acc[0][4 * a + b], powf(d, P.scale));
                        } else {
                            acc[0][4 * a + b] = chain_step<KIND>(q[a], e[b], acc[0][4 * a + b]);
                        }
                    }
            }
        }
        select_tile<TQ, 1>(S, P, row0, cb, acc, [&](int, int r, int& rl, int64_t& col) {
            rl = 4 * tq + (r >> 2);
            col = tile * TE + 4 * te + (r & 3);
        });
    }
    select_finish<TQ>(S, P, row0, cb);
}

// ---------------------------------------------------------------------------------------------
// RotatE: the main loop of count_rotate_kernel (emg_rank.hip) — 64 queries x 64 candidates per workgroup, 4 x 4 per thread, k-tiles of
// RJ complex coordinates with both halves staged in LDS, the k loop stopping at k — and the same selection epilogue.
// ---------------------------------------------------------------------------------------------
constexpr int RJ = 16;

__global__ __launch_bounds__(256) void topn_rotate_kernel(const TopnParams P) {
    __shared__ __attribute__((aligned(16))) float Qs[2 * RJ * TQ];
    __shared__ __attribute__((aligned(16))) float Es[2 * RJ * TE];
    __shared__ SelState<TQ> S;

    const int64_t id = blockIdx.x;
    const int64_t xcd = id & 7, slot = id >> 3;
    const int64_t qb = slot % P.n_qb;
    const int64_t cb = xcd + 8 * (slot / P.n_qb);
    if (cb >= P.n_cb) return;

    const int tid = threadIdx.x;
    const int tq = tid & 15, te = tid >> 4;
    const int lrow = tid & 63, lkq = tid >> 6;  // loader: row lrow, coordinates [4 lkq, 4 lkq + 4) of the tile, both halves
    const int64_t row0 = qb * TQ;
    const int half = P.k_int >> 1;

    sel_init<TQ>(S, tid);

    const float* qptr = P.Q + min(row0 + lrow, P.n_rows - 1) * P.ldq;

    const int64_t tile0 = cb * P.tiles_per_chunk;
    const int64_t tile1 = min(tile0 + (int64_t)P.tiles_per_chunk, P.n_tiles);
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t el = min(tile * TE + lrow, P.n_cand - 1);
        const float* eptr = P.ent + (P.cand ? (int64_t)P.cand[el] : el) * P.ld_ent;
        float16v acc[1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
        for (int j0 = 0; j0 < half; j0 += RJ) {
            float qv[2][4], ev[2][4];   // [0]: real parts, [1]: imaginary parts
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int j = j0 + 4 * lkq + c;
                    qv[h][c] = j < half ? qptr[h * half + j] : 0.f;
                    ev[h][c] = j < half ? eptr[h * half + j] : 0.f;
                }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int kl = h * RJ + 4 * lkq + c;
                    Qs[kl * TQ + lrow] = qv[h][c];
                    Es[kl * TE + lrow] = ev[h][c];
                }
            __syncthreads();
            const int jn = min(RJ, half - j0);
            for (int j = 0; j < jn; ++j) {
                const float4 qr4 = *reinterpret_cast<const float4*>(&Qs[j * TQ + 4 * tq]);
                const float4 qi4 = *reinterpret_cast<const float4*>(&Qs[(RJ + j) * TQ + 4 * tq]);
                const float4 er4 = *reinterpret_cast<const float4*>(&Es[j * TE + 4 * te]);
                const float4 ei4 = *reinterpret_cast<const float4*>(&Es[(RJ + j) * TE + 4 * te]);
                const float qr[4] = {qr4.x, qr4.y, qr4.z, qr4.w}, qi[4] = {qi4.x, qi4.y, qi4.z, qi4.w};
                const float er[4] = {er4.x, er4.y, er4.z, er4.w}, ei[4] = {ei4.x, ei4.y, ei4.z, ei4.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[0][4 * a + b] = rotate_step(qr[a], qi[a], er[b], ei[b], acc[0][4 * a + b]);
            }
        }
        select_tile<TQ, 1>(S, P, row0, cb, acc, [&](int, int r, int& rl, int64_t& col) {
            rl = 4 * tq + (r >> 2);
            col = tile * TE + 4 * te + (r & 3);
        });
    }
    select_finish<TQ>(S, P, row0, cb);
}

// ---------------------------------------------------------------------------------------------
// Phase 2: one wave per query row merges the row's chunk lists (each sorted best first) into the final top N.  A piece of a
// chunk list goes through merge_into only as far as it beats the running tau.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topn_merge_kernel(const uint64_t* __restrict__ lists, int64_t n_rows, int64_t n_cb, int N,
                                                         int32_t* __restrict__ out_ids, float* __restrict__ out_scores) {
    __shared__ uint64_t lst[4][EMG_TOPN_MAX];
    __shared__ uint64_t stage[4][SEL_B];
    __shared__ uint64_t tau_key[4];
    __shared__ float tau_f[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;   // (no workgroup barrier below)
    if (lane == 0) { tau_key[wave] = 0; tau_f[wave] = -INFINITY; }
    wave_sync();
    int L = 0;
    for (int64_t cb = 0; cb < n_cb; ++cb) {
        const uint64_t* src = lists + (row * n_cb + cb) * N;
        for (int p0 = 0; p0 < N; p0 += SEL_B) {
            const uint64_t e = (lane < SEL_B && p0 + lane < N) ? src[p0 + lane] : SEL_PAD;
            const int c = __popcll(__ballot(order_key(e) > tau_key[wave]));   // sorted: the entries that still enter are a prefix
            if (c == 0) break;
            if (lane < SEL_B) stage[wave][lane] = e;
            wave_sync();
            L = merge_into<false>(lst[wave], L, N, stage[wave], c, lane, &tau_f[wave], &tau_key[wave]);
            wave_sync();
            if (c < SEL_B) break;
        }
    }
    for (int i = lane; i < N; i += 64) {
        const uint64_t e = i < L ? lst[wave][i] : SEL_PAD;
        out_ids[row * N + i] = (int32_t)(uint32_t)e;
        out_scores[row * N + i] = __uint_as_float((uint32_t)(e >> 32));
    }
}

int64_t topn_chunk(int64_t ent_chunk) { return cdiv(ent_chunk > 0 ? ent_chunk : TOPN_CHUNK, TOPN_TILE) * TOPN_TILE; }

// bytes of the per-(row, chunk) lists; -1: the product does not fit int64
int64_t topn_list_bytes(int64_t n_rows, int64_t n_cand, int32_t top_n, int64_t ent_chunk) {
    const int64_t n_cb = cdiv(n_cand, topn_chunk(ent_chunk));
    int64_t b;
    if (__builtin_mul_overflow(n_rows, n_cb, &b) || __builtin_mul_overflow(b, (int64_t)top_n * (int64_t)sizeof(uint64_t), &b)) return -1;
    return b;
}

constexpr int64_t TOPN_CHUNK_MAX = (int64_t)1 << 40;

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" int64_t emg_eval_topn_ws_bytes(int64_t n_rows, int64_t n_cand, int32_t top_n, int64_t ent_chunk) {
    EMG_REQUIRE(n_rows >= 0 && n_cand >= 0 && ent_chunk >= 0 && ent_chunk <= TOPN_CHUNK_MAX, "emg_eval_topn_ws_bytes: bad sizes");
    EMG_REQUIRE(top_n >= 1 && top_n <= EMG_TOPN_MAX, "emg_eval_topn_ws_bytes: top_n %d outside [1, %d]", (int)top_n, EMG_TOPN_MAX);
    const int64_t b = topn_list_bytes(n_rows, n_cand, top_n, ent_chunk);
    EMG_REQUIRE(b >= 0, "emg_eval_topn_ws_bytes: the workspace size does not fit 64 bits");
    return b;
}

extern "C" int emg_eval_topn(int model, const float* Q, int64_t ldq, int64_t n_rows, const float* ent, int64_t n_cand,
                             int64_t ld_ent, const int32_t* cand, int64_t ent_offset, int32_t k_int, float scale, int32_t top_n,
                             const int64_t* excl_ptr, const int32_t* excl_idx, int64_t ent_chunk, void* ws, int64_t ws_bytes,
                             int32_t* out_ids, float* out_scores, void* stream) {
    model = chain_model(model);
    EMG_REQUIRE(model >= 0 && model <= EMG_ROTATE, "emg_eval_topn: unknown model id %d", model);
    EMG_REQUIRE(model != EMG_ROTATE || k_int % 2 == 0, "emg_eval_topn: EMG_ROTATE: odd k_int %d", (int)k_int);
    EMG_REQUIRE(top_n >= 1 && top_n <= EMG_TOPN_MAX, "emg_eval_topn: top_n %d outside [1, %d]", (int)top_n, EMG_TOPN_MAX);
    EMG_REQUIRE(n_rows >= 0 && n_cand >= 0 && k_int > 0 && ldq >= k_int && ld_ent >= k_int && ent_chunk >= 0 &&
                ent_chunk <= TOPN_CHUNK_MAX && ws_bytes >= 0, "emg_eval_topn: bad sizes");
    EMG_REQUIRE(ent_offset >= 0 && ent_offset <= INT32_MAX && n_cand <= INT32_MAX - ent_offset, "emg_eval_topn: entity ids must fit int32");
    EMG_REQUIRE(model != EMG_TRANSE_P || scale > 0.f, "EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive");
    if (n_rows == 0) return EMG_OK;
    EMG_REQUIRE(out_ids && out_scores, "emg_eval_topn: null output");
    EMG_REQUIRE(n_cand == 0 || (Q && ent), "emg_eval_topn: null pointer");
    const int64_t need = topn_list_bytes(n_rows, n_cand, top_n, ent_chunk);
    EMG_REQUIRE(need >= 0 && need <= ws_bytes && (need == 0 || ws), "emg_eval_topn: workspace of %lld bytes, emg_eval_topn_ws_bytes asks for %lld",
                (long long)ws_bytes, (long long)need);
    EMG_REQUIRE(need == 0 || (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "emg_eval_topn: the workspace must be 8-byte aligned");
    EMG_REQUIRE(cdiv(n_rows, 4) < ((int64_t)1 << 31), "emg_eval_topn: grid too large");
    hipStream_t st = (hipStream_t)stream;
    TopnParams P{};
    P.Q = Q; P.ldq = ldq; P.n_rows = n_rows; P.ent = ent; P.n_cand = n_cand; P.ld_ent = ld_ent; P.cand = cand; P.ent_offset = ent_offset;
    P.k_int = k_int; P.scale = scale; P.model = model; P.top_n = top_n; P.excl_ptr = excl_ptr; P.excl_idx = excl_idx;
    P.lists = static_cast<uint64_t*>(ws);
    const int64_t chunk = topn_chunk(ent_chunk);
    P.n_cb = cdiv(n_cand, chunk);
    if (n_cand > 0) {
        const bool dot = model == EMG_DISTMULT || model == EMG_COMPLEX || model == EMG_HOLE;
        const int bm = dot ? BM : TQ, bn = dot ? BNW : TE;
        P.n_qb = cdiv(n_rows, bm);
        P.n_tiles = cdiv(n_cand, bn);
        P.tiles_per_chunk = (int32_t)(chunk / bn);
        const int64_t blocks = 8 * P.n_qb * cdiv(P.n_cb, 8);
        EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_eval_topn: grid too large");
        void (*fn)(const TopnParams);
        if (dot) {
            const bool vec = (ldq % 4 == 0) && (ld_ent % 4 == 0) && aligned16(Q) && aligned16(ent) && k_int % 4 == 0;
            fn = vec ? topn_mfma_kernel<true> : topn_mfma_kernel<false>;
        } else if (model == EMG_ROTATE) {
            fn = topn_rotate_kernel;
        } else {
            fn = model == EMG_TRANSE_L1 ? topn_transe_kernel<1> : (model == EMG_TRANSE_L2 ? topn_transe_kernel<2> : topn_transe_kernel<3>);
        }
        hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), 0, st, P);
        EMG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(topn_merge_kernel, dim3((unsigned)cdiv(n_rows, 4)), dim3(256), 0, st, P.lists, n_rows, P.n_cb, (int)top_n, out_ids,
                       out_scores);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
