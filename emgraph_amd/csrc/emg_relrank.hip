// emg_relrank.hip — relation prediction: rank and complete (s, ?, o) against the relation table.
//
// Extends the 1-vs-all scoring of EmbeddingModel.py:1856-1866 (every ENTITY scored against a query) to the third side of a
// triple: every candidate RELATION scored against a (subject, object) pair.  Not in the reference.
//
// ONE TRIPLE, ONE SCORE: the score of (s, r, o) is chain_score(model, Q_obj(s, r), ent[o], k_int, scale) — the query row
// build_queries_kernel (emg_rank.hip) writes for the object side, then the canonical chain of emg_chain.hpp, k ascending over
// the [re | im] layout.  Q_obj depends on the relation, so it cannot be hoisted into a row per pair without changing the bits:
// the kernel builds q per (pair, relation, coordinate) in registers and runs the chain step on it at once.
//
// MAPPING (rel_score_kernel): the relation element of a (relation, coordinate) step is the same for every pair, the pair's s / o
// elements the same for every relation.  Each lane keeps RT = 16 relation accumulators of ONE pair.  Small candidate sets (NG = 1):
// a workgroup takes 256 pairs, one per lane, and walks the candidates in tiles of 16.  From WIDE_MIN candidates on (NG = 4): four
// lanes share a pair, each with its own 16 relations of a tile of 64, and a workgroup takes 64 pairs — a quarter of the pair rows in
// flight per CU and a quarter of the passes over them (the rows are re-streamed once per tile: what bounds the kernel at wide rows).
// k is streamed in slices of KS coordinates: the pairs' subject / object slices are loaded with row-contiguous 16-byte pieces
// and stored k-major in LDS (a lane then reads its own pair's element, conflict-free); the relation tile's slice sits in LDS as
// [k][relation] and is read as 16-byte BROADCASTS (the lanes of a relation group the same address: four relations per LDS
// instruction).  The next slice's global loads fly under the current slice's arithmetic.  ComplEx / HolE run the whole `re` half
// of the chain, then the whole `im` half (two passes over the subject slices).  SimplE (K_SIMPLE) is K_DOT's chain over all 2k columns
// on the half-swapped subject and relation slices — the object-side query swap(rel) o swap(e_s) — then the scale.  A pair's four
// counters live in its lanes for the whole call (NG = 4: summed across the four lanes by shuffles at the end): no atomics, no
// second pass — the filter counts are a membership test of the relation id in the row's ascending exclusion list, made only for a relation that ties with or beats
// the positive.  Either form runs each chain in one lane, k ascending: the same bits.
//
// TOP-N (rel_topn_kernel): the candidate table is small, so the scores of a row chunk are written densely
// (emg_eval_rel_scores_dense) and one wave per row selects from them in the total order of emg_topn.hip.
#include "emg_chain.hpp"

#pragma clang fp contract(off)

namespace emg {
namespace {

constexpr int RP = 256;       // threads per workgroup
constexpr int RT = 16;        // relation accumulators per lane
constexpr int NG_WIDE = 4;    // relation groups of the wide form, taken from WIDE_MIN candidates on
constexpr int WIDE_MIN = 48;

enum { K_DOT = 0, K_L1 = 1, K_L2 = 2, K_P = 3, K_CPLX = 4, K_ROT = 5, K_SIMPLE = 6 };   // the chain of a model
enum { M_COUNT = 0, M_COUNT_LINK = 1, M_DENSE = 2 };

struct RelParams {
    const float* ent; int64_t ld_ent;
    const float* rel; int64_t ld_rel;       // EMG_ROTATE: the [cos | sin] image of rel_image_kernel
    int32_t k_int; float scale; int32_t model; int32_t link;
    const int32_t* test; int64_t n_rows;
    const int32_t* pos_int;
    const int32_t* cand; int32_t n_cand;
    const int64_t* excl_ptr; const int32_t* excl_idx;
    int32_t* cnt_gt; int32_t* cnt_eq; int32_t* fcnt_gt; int32_t* fcnt_eq;
    float* S; int64_t lds;
    int32_t vec, vec_rel;                   // 16-byte pieces of entity / relation rows may be loaded whole
    int32_t half;                           // EMG_SIMPLE: k_int / 2, the half boundary of rows [h | t], [r | r_inv]
};

__device__ __forceinline__ int rel_cmp_int(float score) { return (int)__fmul_rn(score, 100000.0f); }   // EmbeddingModel.py:2010-2014

// the model's final step on a finished chain (as chain_score's returns), of the models of chain KIND
template <int KIND>
__device__ __forceinline__ float rel_chain_final(int model, float scale, float acc) {
    if constexpr (KIND == K_CPLX) return model == EMG_HOLE ? __fmul_rn(acc, scale) : acc;
    else if constexpr (KIND == K_L1 || KIND == K_ROT) return -acc;
    else if constexpr (KIND == K_L2) return -sqrtf(acc);
    else if constexpr (KIND == K_P) return isinf(scale) ? -acc : -powf(acc, 1.0f / scale);
    else if constexpr (KIND == K_SIMPLE) return __fmul_rn(acc, scale);
    else return acc;
}

// id in the ascending list idx[lo, hi)
__device__ __forceinline__ bool rel_member(const int32_t* __restrict__ idx, int64_t lo, int64_t hi, int32_t id) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = idx[mid];
        if (v == id) return true;
        if (v < id) lo = mid + 1; else hi = mid;
    }
    return false;
}

// columns [col, col + 4) of a row, those at or past `lim` as zeros; `whole`: the piece is inside and 16-byte aligned
__device__ __forceinline__ f32x4 rel_load4(const float* __restrict__ row, int col, int lim, bool whole) {
    if (whole) return *reinterpret_cast<const f32x4*>(row + col);
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = col + c < lim ? row[col + c] : 0.f;
    return v;
}

// columns [col, col + 4) of swap(row), the row with its two halves of `half` columns exchanged (EMG_SIMPLE), those at or past 2 half
// as zeros; `whole`: half is a multiple of 4 (a piece never straddles the half boundary), the piece is inside and 16-byte aligned
__device__ __forceinline__ f32x4 rel_load4_swap(const float* __restrict__ row, int col, int half, bool whole) {
    if (whole) return *reinterpret_cast<const f32x4*>(row + (col < half ? col + half : col - half));
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = col + c;
        v[c] = j < 2 * half ? row[j < half ? j + half : j - half] : 0.f;
    }
    return v;
}

// NG relation groups: a wave holds 64 / NG pairs, each in NG lanes, lane g of a pair carrying relations [16 g, 16 g + 16) of the
// tile.  NG = 1: one pair per lane, 256 pairs per workgroup, tiles of 16 relations (small candidate sets).  NG = 4: 64 pairs per
// workgroup, tiles of 64 relations — a quarter of the pair rows in flight per CU and a quarter of the passes over them.
template <int KIND, int MODE, int NG>
__global__ __launch_bounds__(RP, 4) void rel_score_kernel(const RelParams P) {
    constexpr bool CPLX = KIND == K_CPLX || KIND == K_ROT;
    constexpr int NA = KIND == K_ROT ? 4 : (KIND == K_CPLX ? 3 : 2);   // entity slices in LDS: [s | o], [s_re | s_im | o_half], [s_re | s_im | o_re | o_im]
    constexpr int NP = KIND == K_CPLX ? 2 : 1;                          // passes over the coordinates: ComplEx / HolE's re half, then the im half
    constexpr int NC = CPLX ? 2 : 1;                                    // halves of a relation row: [p_r | p_i]
    constexpr int PAIRS = RP / NG;                                      // pairs per workgroup
    constexpr int PW = 64 / NG;                                         // pairs per wave
    constexpr int KS = NG == 1 ? 8 : 16;                                // coordinates per k-slice
    constexpr int KQ = KS / 4;                                          // 4-float pieces of a slice
    constexpr int LDX = PAIRS + (NG == 1 ? 4 : 2);                      // k-major LDS row: the loader's pieces of a 32-lane group land on distinct banks
    constexpr int TR = RT * NG;                                         // relations per tile
    constexpr int XL = PAIRS * KQ / RP;                                 // entity pieces per thread and slice array
    constexpr int RPC = NC * TR * KQ;                                   // relation pieces per slice
    constexpr int RL = (RPC + RP - 1) / RP;                             // ... per thread
    static_assert(PAIRS * KQ % RP == 0 && XL >= 1, "every thread loads whole pieces");
    __shared__ __attribute__((aligned(16))) float Xs[NA][KS][LDX];
    __shared__ __attribute__((aligned(16))) float Rs[NC][KS][TR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * PAIRS;
    const int n = CPLX ? P.k_int >> 1 : P.k_int;   // coordinates of one pass
    const int n_sl = (n + KS - 1) / KS;
    const int n_tiles = (P.n_cand + TR - 1) / TR;
    const int total = n_tiles * NP * n_sl;

    // entity loader: piece x of this thread is piece lq of the slice of workgroup row lr
    const float* srow[XL];
    const float* orow[XL];
#pragma unroll
    for (int x = 0; x < XL; ++x) {
        const int64_t row = min(row0 + (tid + RP * x) / KQ, P.n_rows - 1);
        srow[x] = P.ent + (int64_t)P.test[3 * row + 0] * P.ld_ent;
        orow[x] = P.ent + (int64_t)P.test[3 * row + 2] * P.ld_ent;
    }

    f32x4 xv[NA][XL], rv[RL];
    auto fetch = [&](int tile, int h, int sl) {
#pragma unroll
        for (int x = 0; x < XL; ++x) {
            const int j = sl * KS + 4 * ((tid + RP * x) % KQ);
            const bool whole = P.vec && j + 4 <= n;
            if constexpr (KIND == K_SIMPLE) {   // K_DOT's chain on swap(e_s) and swap(rel): the object-side query, built in registers
                xv[0][x] = rel_load4_swap(srow[x], j, P.half, whole);
                xv[1][x] = rel_load4(orow[x], j, n, whole);
            } else if constexpr (!CPLX) {
                xv[0][x] = rel_load4(srow[x], j, n, whole);
                xv[1][x] = rel_load4(orow[x], j, n, whole);
            } else {
                xv[0][x] = rel_load4(srow[x], j, n, whole);
                xv[1][x] = rel_load4(srow[x] + n, j, n, whole);
                if constexpr (KIND == K_CPLX) {
                    xv[2][x] = rel_load4(orow[x] + h * n, j, n, whole);
                } else {
                    xv[2][x] = rel_load4(orow[x], j, n, whole);
                    xv[NA - 1][x] = rel_load4(orow[x] + n, j, n, whole);
                }
            }
        }
        // relation pieces: piece i = (half, piece of the slice, relation of the tile), the relation fastest
#pragma unroll
        for (int y = 0; y < RL; ++y) {
            const int i = tid + RP * y;
            rv[y] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < RPC) {
                const int c = min(tile * TR + i % TR, P.n_cand - 1);
                const int64_t id = P.cand ? (int64_t)P.cand[c] : (int64_t)c;
                const int j = sl * KS + 4 * ((i / TR) % KQ);
                if constexpr (KIND == K_SIMPLE) rv[y] = rel_load4_swap(P.rel + id * P.ld_rel, j, P.half, P.vec_rel && j + 4 <= n);
                else rv[y] = rel_load4(P.rel + id * P.ld_rel + (i / (TR * KQ)) * n, j, n, P.vec_rel && j + 4 <= n);
            }
        }
    };

    // this lane's pair and relation group
    const int pl = wave * PW + lane % PW, grp = lane / PW;
    const int64_t row = row0 + pl;
    const bool row_ok = row < P.n_rows;
    int pos = 0;
    int64_t ex_lo = 0, ex_hi = 0;
    if constexpr (MODE != M_DENSE) {
        if (row_ok) {
            pos = P.pos_int[row];
            if (P.excl_ptr) { ex_lo = P.excl_ptr[row]; ex_hi = P.excl_ptr[row + 1]; }
        }
    }
    int c_gt = 0, c_eq = 0, f_gt = 0, f_eq = 0;
    const bool ord_inf = KIND == K_P && isinf(P.scale);

    float acc[RT];
    int tile = 0, h = 0, sl = 0;
    if (total > 0) fetch(0, 0, 0);
    for (int it = 0; it < total; ++it) {
        if (h == 0 && sl == 0) {
#pragma unroll
            for (int a = 0; a < RT; ++a) acc[a] = 0.f;
        }
        __syncthreads();   // the previous slice's LDS reads are done
#pragma unroll
        for (int x = 0; x < XL; ++x) {
            const int lq = (tid + RP * x) % KQ, lr = (tid + RP * x) / KQ;
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) Xs[a][4 * lq + c][lr] = xv[a][x][c];
        }
#pragma unroll
        for (int y = 0; y < RL; ++y) {
            const int i = tid + RP * y;
            if (i < RPC) {
#pragma unroll
                for (int c = 0; c < 4; ++c) Rs[i / (TR * KQ)][4 * ((i / TR) % KQ) + c][i % TR] = rv[y][c];
            }
        }
        __syncthreads();
        const int ctile = tile, ch = h;
        const bool tile_done = sl + 1 == n_sl && h + 1 == NP;
        if (++sl == n_sl) { sl = 0; if (++h == NP) { h = 0; ++tile; } }
        if (it + 1 < total) fetch(tile, h, sl);   // flies under the arithmetic below

        const float* rs0 = &Rs[0][0][RT * grp];
        if constexpr (KIND == K_CPLX) {
            // q_re = fmaf(p_r, s_r, -(p_i s_i)) against o_re (pass 0); q_im = fmaf(p_r, s_i, p_i s_r) against o_im (pass 1)
            if (ch == 0) {
#pragma unroll 2
                for (int kk = 0; kk < KS; ++kk) {
                    const float s_r = Xs[0][kk][pl], s_i = Xs[1][kk][pl], o = Xs[2][kk][pl];
#pragma unroll
                    for (int g = 0; g < RT / 4; ++g) {
                        const f32x4 p_r = *reinterpret_cast<const f32x4*>(rs0 + kk * TR + 4 * g);
                        const f32x4 p_i = *reinterpret_cast<const f32x4*>(rs0 + (KS + kk) * TR + 4 * g);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[4 * g + e] = __fmaf_rn(__fmaf_rn(p_r[e], s_r, -__fmul_rn(p_i[e], s_i)), o, acc[4 * g + e]);
                    }
                }
            } else {
#pragma unroll 2
                for (int kk = 0; kk < KS; ++kk) {
                    const float s_r = Xs[0][kk][pl], s_i = Xs[1][kk][pl], o = Xs[2][kk][pl];
#pragma unroll
                    for (int g = 0; g < RT / 4; ++g) {
                        const f32x4 p_r = *reinterpret_cast<const f32x4*>(rs0 + kk * TR + 4 * g);
                        const f32x4 p_i = *reinterpret_cast<const f32x4*>(rs0 + (KS + kk) * TR + 4 * g);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[4 * g + e] = __fmaf_rn(__fmaf_rn(p_r[e], s_i, __fmul_rn(p_i[e], s_r)), o, acc[4 * g + e]);
                    }
                }
            }
        } else if constexpr (KIND == K_ROT) {
#pragma unroll 2
            for (int kk = 0; kk < KS; ++kk) {
                const float s_r = Xs[0][kk][pl], s_i = Xs[1][kk][pl], o_r = Xs[2][kk][pl], o_i = Xs[3][kk][pl];
#pragma unroll
                for (int g = 0; g < RT / 4; ++g) {
                    const f32x4 p_r = *reinterpret_cast<const f32x4*>(rs0 + kk * TR + 4 * g);
                    const f32x4 p_i = *reinterpret_cast<const f32x4*>(rs0 + (KS + kk) * TR + 4 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float q_r = __fmaf_rn(p_r[e], s_r, -__fmul_rn(p_i[e], s_i));
                        const float q_i = __fmaf_rn(p_r[e], s_i, __fmul_rn(p_i[e], s_r));
                        acc[4 * g + e] = rotate_step(q_r, q_i, o_r, o_i, acc[4 * g + e]);
                    }
                }
            }
        } else {
#pragma unroll 2
            for (int kk = 0; kk < KS; ++kk) {
                const float s = Xs[0][kk][pl], o = Xs[1][kk][pl];
#pragma unroll
                for (int g = 0; g < RT / 4; ++g) {
                    const f32x4 p = *reinterpret_cast<const f32x4*>(rs0 + kk * TR + 4 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float& a = acc[4 * g + e];
                        if constexpr (KIND == K_DOT || KIND == K_SIMPLE) {
                            a = __fmaf_rn(__fmul_rn(p[e], s), o, a);
                        } else if constexpr (KIND == K_P) {
                            const float d = fabsf(__fsub_rn(__fadd_rn(s, p[e]), o));
                            a = ord_inf ? fmaxf(a, d) : __fadd_rn(a, powf(d, P.scale));
                        } else {
                            a = chain_step<KIND>(__fadd_rn(s, p[e]), o, a);   // K_L1 / K_L2 are chain_step's kinds 1 / 2
                        }
                    }
                }
            }
        }

        if (tile_done) {   // (workgroup-uniform)
#pragma unroll
            for (int a = 0; a < RT; ++a) {
                const int c = ctile * TR + RT * grp + a;
                if (c < P.n_cand && row_ok) {
                    const float v = rel_chain_final<KIND>(P.model, P.scale, acc[a]);
                    if constexpr (MODE == M_DENSE) {
                        P.S[row * P.lds + c] = v;
                    } else {
                        const int ci = MODE == M_COUNT_LINK ? link_cmp_int(P.link, v) : rel_cmp_int(v);
                        const bool gt = ci > pos, eq = ci == pos;
                        c_gt += gt; c_eq += eq;
                        if ((gt || eq) && ex_lo < ex_hi && rel_member(P.excl_idx, ex_lo, ex_hi, P.cand ? P.cand[c] : c)) {
                            f_gt += gt; f_eq += eq;
                        }
                    }
                }
            }
        }
    }
    if constexpr (MODE != M_DENSE) {
        // the NG lanes of a pair sit PW lanes apart in the wave: sum their counters
#pragma unroll
        for (int d = PW; d < 64; d <<= 1) {
            c_gt += __shfl_xor(c_gt, d, 64); c_eq += __shfl_xor(c_eq, d, 64);
            f_gt += __shfl_xor(f_gt, d, 64); f_eq += __shfl_xor(f_eq, d, 64);
        }
        if (row_ok && grp == 0) { P.cnt_gt[row] = c_gt; P.cnt_eq[row] = c_eq; P.fcnt_gt[row] = f_gt; P.fcnt_eq[row] = f_eq; }
    }
}

// RotatE: the [cos | sin] image of the phase table, the sincosf call of build_queries_kernel once per (relation, coordinate)
__global__ void rel_image_kernel(const float* __restrict__ rel, int64_t n_rel, int64_t ld_rel, int n, float* __restrict__ img,
                                 int64_t ld_img) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rel * n) return;
    const int64_t r = t / n;
    const int c = (int)(t - r * n);
    float p_r, p_i;
    sincosf(rel[r * ld_rel + c], &p_i, &p_r);
    img[r * ld_img + c] = p_r;
    img[r * ld_img + n + c] = p_i;
}

// the total order of emg_topn.hip, restated: larger key = earlier; higher score first, -0 == +0, NaN below -inf, equal scores
// by ascending id (ids are < 2^31: the low word is never 0, so 0 is "nothing")
__device__ __forceinline__ uint64_t rel_order_key(float score, int32_t id) {
    const uint32_t u = __float_as_uint(score);
    uint32_t k;
    if ((u & 0x7fffffffu) > 0x7f800000u) k = 0u;
    else if (u == 0x80000000u) k = 0x80000000u;
    else k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)k << 32) | (uint32_t)~(uint32_t)id;
}

// One wave per row: repeat "the largest key below the last one taken" over the row's dense scores.  Keys are unique (the id is
// part of the key), so every round has one owner lane, which writes the slot; a winner in the row's exclusion list takes no slot.
__global__ __launch_bounds__(256) void rel_topn_kernel(const float* __restrict__ S, int64_t lds, int64_t n_rows, int n_cand,
                                                       const int32_t* __restrict__ cand, const int64_t* __restrict__ excl_ptr,
                                                       const int32_t* __restrict__ excl_idx, int top_n, int32_t* __restrict__ out_ids,
                                                       float* __restrict__ out_scores) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;   // (no workgroup barrier below)
    const float* srow = S + row * lds;
    int64_t ex_lo = 0, ex_hi = 0;
    if (excl_ptr) { ex_lo = excl_ptr[row]; ex_hi = excl_ptr[row + 1]; }
    uint64_t last = ~0ull;
    int taken = 0;
    while (taken < top_n) {
        uint64_t best = 0;
        float best_score = 0.f;
        for (int j = lane; j < n_cand; j += 64) {
            const float v = srow[j];
            const uint64_t key = rel_order_key(v, cand ? cand[j] : j);
            if (key < last && key > best) { best = key; best_score = v; }
        }
        uint64_t m = best;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t other = __shfl_xor(m, d, 64);
            m = other > m ? other : m;
        }
        if (m == 0) break;   // the row is exhausted
        last = m;
        const int32_t id = (int32_t)~(uint32_t)m;
        if (rel_member(excl_idx, ex_lo, ex_hi, id)) continue;   // (wave-uniform)
        if (best == m) { out_ids[row * top_n + taken] = id; out_scores[row * top_n + taken] = best_score; }
        ++taken;
    }
    for (int i = taken + lane; i < top_n; i += 64) { out_ids[row * top_n + i] = -1; out_scores[row * top_n + i] = -INFINITY; }
}

int rel_kind(int model) {
    switch (model) {
        case EMG_TRANSE_L1: return K_L1;
        case EMG_TRANSE_L2: return K_L2;
        case EMG_TRANSE_P: return K_P;
        case EMG_DISTMULT: return K_DOT;
        case EMG_ROTATE: return K_ROT;
        case EMG_SIMPLE: return K_SIMPLE;
        default: return K_CPLX;
    }
}

template <int MODE, int NG>
void (*rel_kernel(int kind))(const RelParams) {
    switch (kind) {
        case K_DOT: return rel_score_kernel<K_DOT, MODE, NG>;
        case K_L1: return rel_score_kernel<K_L1, MODE, NG>;
        case K_L2: return rel_score_kernel<K_L2, MODE, NG>;
        case K_P: return rel_score_kernel<K_P, MODE, NG>;
        case K_CPLX: return rel_score_kernel<K_CPLX, MODE, NG>;
        case K_SIMPLE: return rel_score_kernel<K_SIMPLE, MODE, NG>;
        default: return rel_score_kernel<K_ROT, MODE, NG>;
    }
}

template <int NG>
void (*rel_kernel_mode(int mode, int kind))(const RelParams) {
    return mode == M_DENSE ? rel_kernel<M_DENSE, NG>(kind) : (mode == M_COUNT_LINK ? rel_kernel<M_COUNT_LINK, NG>(kind) : rel_kernel<M_COUNT, NG>(kind));
}

// what the count and the dense entry points check alike, and the launch
int rel_launch(const char* what, int mode, RelParams& P, int64_t n_ent, int64_t n_rel, void* stream) {
    EMG_REQUIRE((P.model >= 0 && P.model <= EMG_ROTATE) || P.model == EMG_SIMPLE, "%s: unknown model id %d", what, (int)P.model);
    const bool cplx = P.model == EMG_COMPLEX || P.model == EMG_HOLE || P.model == EMG_ROTATE;
    const bool halves = cplx || P.model == EMG_SIMPLE;   // rows of two halves: 16-byte pieces need a half boundary at a multiple of 4
    EMG_REQUIRE(P.k_int > 0 && (!cplx || P.k_int % 2 == 0), "%s: k_int %d (a complex model's is even)", what, (int)P.k_int);
    EMG_REQUIRE(P.model != EMG_SIMPLE || P.k_int % 2 == 0, "%s: EMG_SIMPLE: odd k_int %d (rows [h | t], [r | r_inv])", what, (int)P.k_int);
    P.half = P.k_int / 2;
    EMG_REQUIRE(P.n_rows >= 0 && n_ent >= 1 && n_rel >= 1 && P.ld_ent >= P.k_int && P.ld_rel >= P.k_int, "%s: bad sizes", what);
    EMG_REQUIRE(P.n_cand >= 0 && (P.cand || P.n_cand <= n_rel), "%s: n_cand %d outside [0, n_rel] without a candidate list", what,
                (int)P.n_cand);
    EMG_REQUIRE(P.model != EMG_TRANSE_P || P.scale > 0.f, "EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive");
    EMG_REQUIRE((P.excl_ptr == nullptr) == (P.excl_idx == nullptr) || P.excl_ptr, "%s: excl_idx without excl_ptr", what);
    if (P.n_rows == 0) return EMG_OK;
    EMG_REQUIRE(P.ent && P.rel && P.test, "%s: null pointer", what);
    const bool wide = P.n_cand >= WIDE_MIN;   // (the two forms give the same bits: each chain is one lane's, whatever the mapping)
    const int64_t blocks = cdiv(P.n_rows, wide ? RP / NG_WIDE : RP);
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "%s: grid too large", what);
    P.vec = aligned16(P.ent) && P.ld_ent % 4 == 0 && (!halves || P.half % 4 == 0);
    P.vec_rel = aligned16(P.rel) && P.ld_rel % 4 == 0 && (!halves || P.half % 4 == 0);
    void (*fn)(const RelParams) = wide ? rel_kernel_mode<NG_WIDE>(mode, rel_kind(P.model)) : rel_kernel_mode<1>(mode, rel_kind(P.model));
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(RP), 0, (hipStream_t)stream, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" int emg_eval_rel_rotate_image(const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float* img, int64_t ld_img,
                                         void* stream) {
    EMG_REQUIRE(n_rel >= 0 && k_int > 0 && k_int % 2 == 0 && ld_rel >= k_int / 2 && ld_img >= k_int, "emg_eval_rel_rotate_image: bad sizes");
    if (n_rel == 0) return EMG_OK;
    EMG_REQUIRE(rel && img, "emg_eval_rel_rotate_image: null pointer");
    const int64_t blocks = cdiv(n_rel * (k_int / 2), 256);
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_eval_rel_rotate_image: grid too large");
    hipLaunchKernelGGL(rel_image_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rel, n_rel, ld_rel, (int)(k_int / 2), img,
                       ld_img);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_eval_rel_count(int model, int32_t link, const float* ent, int64_t n_ent, int64_t ld_ent, const float* rel, int64_t n_rel,
                                  int64_t ld_rel, int32_t k_int, float scale, const int32_t* test, int64_t n_rows, const int32_t* pos_int,
                                  const int32_t* cand_rel, int64_t n_cand, const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* cnt_gt,
                                  int32_t* cnt_eq, int32_t* fcnt_gt, int32_t* fcnt_eq, void* stream) {
    EMG_REQUIRE(link >= EMG_LINK_LINEAR && link <= EMG_LINK_SOFTPLUS, "emg_eval_rel_count: unknown link %d", (int)link);
    EMG_REQUIRE(n_cand >= 0 && n_cand <= INT32_MAX - RT, "emg_eval_rel_count: n_cand must fit int32");
    EMG_REQUIRE(n_rows <= 0 || (pos_int && cnt_gt && cnt_eq && fcnt_gt && fcnt_eq), "emg_eval_rel_count: null pointer");
    RelParams P{};
    P.ent = ent; P.ld_ent = ld_ent; P.rel = rel; P.ld_rel = ld_rel; P.k_int = k_int; P.scale = scale; P.model = model; P.link = link;
    P.test = test; P.n_rows = n_rows; P.pos_int = pos_int; P.cand = cand_rel; P.n_cand = (int32_t)n_cand;
    P.excl_ptr = excl_ptr; P.excl_idx = excl_idx; P.cnt_gt = cnt_gt; P.cnt_eq = cnt_eq; P.fcnt_gt = fcnt_gt; P.fcnt_eq = fcnt_eq;
    return rel_launch("emg_eval_rel_count", link == EMG_LINK_LINEAR ? M_COUNT : M_COUNT_LINK, P, n_ent, n_rel, stream);
}

extern "C" int emg_eval_rel_scores_dense(int model, const float* ent, int64_t n_ent, int64_t ld_ent, const float* rel, int64_t n_rel,
                                         int64_t ld_rel, int32_t k_int, float scale, const int32_t* test, int64_t n_rows,
                                         const int32_t* cand_rel, int64_t n_cand, float* S, int64_t lds, void* stream) {
    EMG_REQUIRE(n_cand >= 0 && n_cand <= INT32_MAX - RT && lds >= n_cand, "emg_eval_rel_scores_dense: bad sizes");
    EMG_REQUIRE(n_rows <= 0 || n_cand == 0 || S, "emg_eval_rel_scores_dense: null output");
    RelParams P{};
    P.ent = ent; P.ld_ent = ld_ent; P.rel = rel; P.ld_rel = ld_rel; P.k_int = k_int; P.scale = scale; P.model = model;
    P.test = test; P.n_rows = n_rows; P.cand = cand_rel; P.n_cand = (int32_t)n_cand; P.S = S; P.lds = lds;
    return rel_launch("emg_eval_rel_scores_dense", M_DENSE, P, n_ent, n_rel, stream);
}

extern "C" int emg_eval_rel_topn(const float* S, int64_t lds, int64_t n_rows, int64_t n_cand, const int32_t* cand_rel,
                                 const int64_t* excl_ptr, const int32_t* excl_idx, int32_t top_n, int32_t* ids, float* scores, void* stream) {
    EMG_REQUIRE(top_n >= 1 && top_n <= EMG_TOPN_MAX, "emg_eval_rel_topn: top_n %d outside [1, %d]", (int)top_n, EMG_TOPN_MAX);
    EMG_REQUIRE(n_rows >= 0 && n_cand >= 0 && n_cand <= INT32_MAX - 64 && lds >= n_cand, "emg_eval_rel_topn: bad sizes");
    EMG_REQUIRE((excl_ptr == nullptr) == (excl_idx == nullptr) || excl_ptr, "emg_eval_rel_topn: excl_idx without excl_ptr");
    if (n_rows == 0) return EMG_OK;
    EMG_REQUIRE(ids && scores && (n_cand == 0 || S), "emg_eval_rel_topn: null pointer");
    EMG_REQUIRE(cdiv(n_rows, 4) < ((int64_t)1 << 31), "emg_eval_rel_topn: grid too large");
    hipLaunchKernelGGL(rel_topn_kernel, dim3((unsigned)cdiv(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, S, lds, n_rows, (int)n_cand,
                       cand_rel, excl_ptr, excl_idx, (int)top_n, ids, scores);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
