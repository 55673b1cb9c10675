// emg_relneg.hip — relation negatives: the relation of a positive replaced (DESIGN.md 0 A-28, 4.1 "Relation negatives";
// include/emgraph_hip.h has the contract).
//
// Draw j of the positive i = (s, p, o) is (s, p', o), p' = idx + (idx >= p) with idx = codes[j B + i] in [0, n_rel - 1): the two entity
// rows are the positive's own, only the relation row changes.  Per positive the work is eta serial chains over two shared rows; the
// relation table is small (L2) and every lane gathers its own row of it.
//   forward   a workgroup = (run of positives, slice of their items); an item is a draw, or — last, when scores_pos is asked for — the
//             positive itself (p' = p).  A lane carries up to kRnItems (positive, item) chains, the positive fastest across lanes.  The
//             run's s / o rows pass through LDS in slices of kRnSlice coordinates, rows of kRnSlice + 1 words (lanes of a wave read
//             distinct banks); a lane reads its relation row from global memory in the same steps, 16 bytes at a time where it can.
//             One chain = one lane, k ascending: the expressions of emg_relrank.hip::rel_score_kernel, so a score has the bits
//             emg_eval_rel_scores_dense gives for the same (pair, relation).  ComplEx / HolE run the whole `re` half of the chain,
//             then the whole `im` half: two passes over the slices.
//   backward  a gradient column depends on that column of the three rows (complex models, SimplE: on the column and its partner in
//             the other half) and on per-triple scalars only: a thread = (positive, group of W columns), rows read and written with
//             consecutive threads on consecutive columns.  It keeps its s / o columns in registers, walks the draws in ascending j,
//             writes each draw's relation row at once and carries the two entity sums in double, rounded once at the end.  Fixed
//             order, no atomics: two runs give the same bits.  A term is, operation for operation, what emg_train_backward_ex
//             (fused_loss = -1, eta = 0) stores for the triple taken as a positive (emg_score_kernels.hpp::finish_grads on zero accumulators,
//             the generic kernels of emg_score.hip and emg_simple.hip).
//             The eta B relation rows are this kernel's byte floor (0.5 GB at bench.py's default shape): they cannot wait in the
//             256 MB Infinity Cache for the apply, and stored plainly they would push out the entity contribution rows the apply does
//             find there (residency table: a plain store stream leaves 0.15 - 0.30 of a resident set, an `nt` one
//             0.99 - 1.00) — so they are stored `nt`; the 2 B entity rows (a tenth of that) plainly.
// An idx outside [0, n_rel - 1) is never followed (the lane takes relation 0) and raises a device flag the entry point reads back.
#include <cmath>
#include <type_traits>

#include "emg_chain.hpp"

// explicit operations only (the canonical chain; emg_chain.hpp sets the same)
#pragma clang fp contract(off)

namespace emg {
namespace {

constexpr int kRnThreads = 256;
constexpr int kRnItems = 2;        // (positive, item) chains a forward lane carries
constexpr int kRnMaxPos = 32;      // positives of a forward workgroup, at most
constexpr int kRnSlice = 32;       // coordinates per LDS slice (tests/test_relation_negatives.py names it: widths past two slices)
constexpr int kRnLd = kRnSlice + 1;

enum { RK_DOT = 0, RK_L1 = 1, RK_L2 = 2, RK_P = 3, RK_CPLX = 4, RK_ROT = 5, RK_SIMPLE = 6 };   // the chain of a model (emg_relrank.hip's kinds)

__device__ int32_t g_relneg_bad;   // raised by a lane that met an idx outside [0, n_rel - 1)

struct RelnegParams {
    int32_t model, k_int; float scale; int32_t eta;
    const float* ent; int64_t ld_ent; const float* rel; int64_t n_rel; int64_t ld_rel;
    const int32_t* pos; int64_t B; const int32_t* codes;
    float* scores_pos; float* scores_neg;
    const float* g_pos; const float* g_neg; const float* raw_pos; const float* raw_neg;
    float* contrib_ent; float* contrib_rel; int64_t ldc; int32_t* dest_ent; int32_t* dest_rel;
    int32_t n_items;    // forward: eta, + 1 with scores_pos (the last item is the positive)
    int32_t npos;       // forward: positives per workgroup
    int32_t nsl;        // forward: items per slice
    int32_t n_slices;   // forward: slices per run
    int32_t nq;         // backward: column groups per positive
};

// p' of a draw; an idx outside the range raises the flag and is taken as 0
__device__ __forceinline__ int relneg_shift(int32_t idx, int32_t p, int64_t n_rel) {
    if ((uint32_t)idx >= (uint32_t)(n_rel - 1)) { g_relneg_bad = 1; idx = 0; }
    return idx + (idx >= p ? 1 : 0);
}

template <int W>
__device__ __forceinline__ void rn_load(const float* __restrict__ row, int c, float (&v)[W]) {
    if constexpr (W == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(row + c);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = row[c];
    }
}

// RotatE's chain step, emg_chain.hpp::rotate_step's values: the two squares are kept apart from their sum.  The `_rn` operations come
// from the device library with its own contraction flags, which the pragma above does not reach: left to itself the compiler fuses
// fmul + fadd here into v_fmac_f32 (it does not in rel_score_kernel, whose packed multiplications keep them apart), one rounding
// less than the canonical chain and a last-bit difference in one score of a few thousand.
__device__ __forceinline__ float rn_unfused(float x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float rn_rotate_step(float q_re, float q_im, float e_re, float e_im, float acc) {
    const float dr = __fsub_rn(q_re, e_re), di = __fsub_rn(q_im, e_im);
    const float rr = rn_unfused(__fmul_rn(dr, dr)), ii = rn_unfused(__fmul_rn(di, di));
    return __fadd_rn(acc, sqrtf(__fadd_rn(rr, ii)));
}

template <int KIND>
__device__ __forceinline__ float rn_final(int model, float scale, float acc) {
    if constexpr (KIND == RK_CPLX) return model == EMG_HOLE ? __fmul_rn(acc, scale) : acc;
    else if constexpr (KIND == RK_L1 || KIND == RK_ROT) return -acc;
    else if constexpr (KIND == RK_L2) return -sqrtf(acc);
    else if constexpr (KIND == RK_P) return isinf(scale) ? -acc : -powf(acc, 1.0f / scale);
    else if constexpr (KIND == RK_SIMPLE) return __fmul_rn(acc, scale);
    else return acc;
}

// VEC: 16-byte pieces of entity and relation rows (the entry point has checked alignment, strides and the column count)
template <int KIND, bool VEC>
__global__ __launch_bounds__(kRnThreads) void relneg_forward_kernel(const RelnegParams P) {
    constexpr bool CPLX = KIND == RK_CPLX || KIND == RK_ROT;
    constexpr int NA = KIND == RK_ROT ? 4 : (KIND == RK_CPLX ? 3 : 2);   // entity slices in LDS: [s | o], [s_re | s_im | o_half], [s_re | s_im | o_re | o_im]
    constexpr int NP = KIND == RK_CPLX ? 2 : 1;                          // passes over the coordinates
    constexpr int W = VEC ? 4 : 1;
    constexpr int GW = kRnSlice / W;                                     // pieces per LDS row
    __shared__ float Xs[NA][kRnMaxPos][kRnLd];
    __shared__ int ids[3][kRnMaxPos];

    const int tid = threadIdx.x;
    const int64_t run = blockIdx.x / P.n_slices;
    const int sl = (int)(blockIdx.x - run * P.n_slices);
    const int64_t i0 = run * P.npos;
    const int np = (int)(P.B - i0 < P.npos ? P.B - i0 : P.npos);
    const int e0 = sl * P.nsl;
    const int ne = P.n_items - e0 < P.nsl ? P.n_items - e0 : P.nsl;
    const int n = CPLX ? P.k_int >> 1 : P.k_int;   // coordinates of one pass
    const int half = P.k_int >> 1;                  // RK_SIMPLE: the half boundary of rows [h | t], [r | r_inv]
    const bool ord_inf = KIND == RK_P && isinf(P.scale);

    for (int t = tid; t < np; t += kRnThreads) {
        ids[0][t] = P.pos[3 * (i0 + t)];
        ids[1][t] = P.pos[3 * (i0 + t) + 1];
        ids[2][t] = P.pos[3 * (i0 + t) + 2];
    }
    __syncthreads();

    float acc[kRnItems];
    const float* rrow[kRnItems];
    int ip[kRnItems], ie[kRnItems];
    bool act[kRnItems];
#pragma unroll
    for (int r = 0; r < kRnItems; ++r) {
        const int it = tid + kRnThreads * r;
        const int el = it / np;
        ip[r] = it - el * np;
        ie[r] = e0 + el;
        act[r] = el < ne;
        acc[r] = 0.f;
        rrow[r] = P.rel;
        if (act[r]) {
            const int p = ids[1][ip[r]];
            const int pp = ie[r] < P.eta ? relneg_shift(P.codes[(int64_t)ie[r] * P.B + i0 + ip[r]], p, P.n_rel) : p;
            rrow[r] = P.rel + (int64_t)pp * P.ld_rel;
        }
    }

    for (int h = 0; h < NP; ++h) {
        for (int c0 = 0; c0 < n; c0 += kRnSlice) {
            const int nc = n - c0 < kRnSlice ? n - c0 : kRnSlice;
            __syncthreads();   // the previous slice's LDS reads are done
            for (int t = tid; t < NA * np * GW; t += kRnThreads) {
                const int a = t / (np * GW), rem = t - a * (np * GW);
                const int i = rem / GW, lc = (rem - i * GW) * W;
                if (lc >= nc) continue;
                const int c = c0 + lc;
                const float* row = P.ent + (int64_t)ids[(a == NA - 1 || (KIND == RK_ROT && a == 2)) ? 2 : 0][i] * P.ld_ent;
                int sc;
                if constexpr (KIND == RK_SIMPLE) sc = a == 0 ? (c < half ? c + half : c - half) : c;   // swap(e_s): the object-side query's operand
                else if constexpr (KIND == RK_CPLX) sc = a == 0 ? c : (a == 1 ? n + c : h * n + c);
                else if constexpr (KIND == RK_ROT) sc = (a & 1) ? n + c : c;
                else sc = c;
                float v[W];
                rn_load<W>(row, sc, v);
#pragma unroll
                for (int w = 0; w < W; ++w) Xs[a][i][lc + w] = v[w];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kRnItems; ++r) {
                if (!act[r]) continue;
                const int i = ip[r];
                float a_ = acc[r];
                for (int lc = 0; lc < nc; lc += W) {
                    const int c = c0 + lc;
                    float pr[W], pi[W];
                    if constexpr (KIND == RK_SIMPLE) {
                        rn_load<W>(rrow[r], c < half ? c + half : c - half, pr);   // swap(rel)
                    } else {
                        rn_load<W>(rrow[r], c, pr);
                        if constexpr (KIND == RK_CPLX) rn_load<W>(rrow[r], n + c, pi);
                    }
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        if constexpr (KIND == RK_DOT || KIND == RK_SIMPLE) {
                            a_ = __fmaf_rn(__fmul_rn(pr[w], Xs[0][i][lc + w]), Xs[1][i][lc + w], a_);
                        } else if constexpr (KIND == RK_P) {
                            const float d = fabsf(__fsub_rn(__fadd_rn(Xs[0][i][lc + w], pr[w]), Xs[1][i][lc + w]));
                            a_ = ord_inf ? fmaxf(a_, d) : __fadd_rn(a_, powf(d, P.scale));
                        } else if constexpr (KIND == RK_L1 || KIND == RK_L2) {
                            a_ = chain_step<KIND>(__fadd_rn(Xs[0][i][lc + w], pr[w]), Xs[1][i][lc + w], a_);
                        } else if constexpr (KIND == RK_CPLX) {
                            const float s_r = Xs[0][i][lc + w], s_i = Xs[1][i][lc + w], o = Xs[2][i][lc + w];
                            const float q = h == 0 ? __fmaf_rn(pr[w], s_r, -__fmul_rn(pi[w], s_i)) : __fmaf_rn(pr[w], s_i, __fmul_rn(pi[w], s_r));
                            a_ = __fmaf_rn(q, o, a_);
                        } else {   // RK_ROT: the relation row holds phases
                            float p_r, p_i;
                            sincosf(pr[w], &p_i, &p_r);
                            const float s_r = Xs[0][i][lc + w], s_i = Xs[1][i][lc + w];
                            const float q_r = __fmaf_rn(p_r, s_r, -__fmul_rn(p_i, s_i));
                            const float q_i = __fmaf_rn(p_r, s_i, __fmul_rn(p_i, s_r));
                            a_ = rn_rotate_step(q_r, q_i, Xs[2][i][lc + w], Xs[3][i][lc + w], a_);
                        }
                    }
                }
                acc[r] = a_;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kRnItems; ++r) {
        if (!act[r]) continue;
        const float v = rn_final<KIND>(P.model, P.scale, acc[r]);
        if (ie[r] < P.eta) P.scores_neg[(int64_t)ie[r] * P.B + i0 + ip[r]] = v;
        else P.scores_pos[i0 + ip[r]] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// the upstream coefficient rn_term takes, from dL/dscore and the triple's raw score (inner_coef of emg_score_kernels.hpp; the generic
// kernels' own first lines)
template <int MODEL>
__device__ __forceinline__ float rn_coef(float g, float raw, float scale, float* nrm) {
    *nrm = 0.f;
    if constexpr (MODEL == EMG_TRANSE_L2) { const float nr = -raw; return nr > 0.f ? g / nr : 0.f; }
    else if constexpr (MODEL == EMG_TRANSE_P) { *nrm = -raw; return g; }
    else if constexpr (MODEL == EMG_HOLE) return g * scale;
    else if constexpr (MODEL == EMG_SIMPLE) return __fmul_rn(g, scale);
    else return g;
}

// One column (two-half models: column c of the first half and its partner c of the second, [0] and [1]) of the gradient rows
// emg_train_backward_ex(fused_loss = -1, eta = 0) stores for the triple (a, p, b): the same operations in the same order.  The tuned
// models: emg_score_kernels.hpp::finish_grads with its two accumulators A_o = A_s = z = +0 (no negatives) — the coefficient goes into
// the entity row first (b = z + gi o), then the relation multiplies it; the generic ones: their kernels' stores.
//   gi / nrm: rn_coef's;  EMG_ROTATE: p[0] is the phase
template <int MODEL>
__device__ __forceinline__ void rn_term(const float (&a)[2], const float (&p)[2], const float (&b)[2], float gi, float nrm, float ord,
                                        float (&ga)[2], float (&gp)[2], float (&gb)[2]) {
    const float z = 0.f;
    if constexpr (MODEL == EMG_TRANSE_L1 || MODEL == EMG_TRANSE_L2) {
        const float d = (a[0] + p[0]) - b[0];
        const float t = MODEL == EMG_TRANSE_L1 ? gi * sgnf(d) : gi * d;
        ga[0] = -z - t; gp[0] = -z - z - t; gb[0] = z + t;
    } else if constexpr (MODEL == EMG_TRANSE_P) {
        const float d = (a[0] + p[0]) - b[0];
        const float ad = fabsf(d);
        float u = 0.f;
        if (nrm != 0.f && ad != 0.f) u = (d > 0.f ? 1.f : -1.f) * powf(ad, ord - 1.f) / powf(nrm, ord - 1.f);
        const float v = gi * u;
        ga[0] = -v; gp[0] = -v; gb[0] = v;
    } else if constexpr (MODEL == EMG_DISTMULT) {
        const float bo = __fmaf_rn(gi, b[0], z), bs = __fmaf_rn(gi, a[0], z);   // the effective object / subject row
        ga[0] = p[0] * bo;
        gb[0] = p[0] * bs;
        gp[0] = __fmaf_rn(a[0], bo, z * b[0]);
    } else if constexpr (MODEL == EMG_ROTATE) {
        float cn, sn;
        sincosf(p[0], &sn, &cn);
        const float wr = __fmaf_rn(a[0], cn, -__fmul_rn(a[1], sn));
        const float wi = __fmaf_rn(a[0], sn, __fmul_rn(a[1], cn));
        const float dr = __fsub_rn(wr, b[0]), di = __fsub_rn(wi, b[1]);
        const float m = sqrtf(__fmaf_rn(dr, dr, __fmul_rn(di, di)));
        const float ur = m > 0.f ? dr / m : 0.f, ui = m > 0.f ? di / m : 0.f;
        ga[0] = -gi * (ur * cn + ui * sn); ga[1] = -gi * (ui * cn - ur * sn);
        gb[0] = gi * ur; gb[1] = gi * ui;
        gp[0] = gi * (ur * wi - ui * wr); gp[1] = 0.f;
    } else if constexpr (MODEL == EMG_SIMPLE) {   // gi = g * scale;  [0] = the h / r half, [1] = the t / r_inv half
        ga[0] = __fmul_rn(gi, __fmul_rn(p[0], b[1])); ga[1] = __fmul_rn(gi, __fmul_rn(p[1], b[0]));
        gb[1] = __fmul_rn(gi, __fmul_rn(p[0], a[0])); gb[0] = __fmul_rn(gi, __fmul_rn(p[1], a[1]));
        gp[0] = __fmul_rn(gi, __fmul_rn(a[0], b[1])); gp[1] = __fmul_rn(gi, __fmul_rn(a[1], b[0]));
    } else {   // ComplEx / HolE
        const float sr = a[0], si = a[1], pr = p[0], pi = p[1], orr = b[0], oi = b[1];
        const float br = __fmaf_rn(gi, orr, z), bi = __fmaf_rn(gi, oi, z);   // b = Ao + gi o
        const float ar = __fmaf_rn(gi, sr, z), ai = __fmaf_rn(gi, si, z);    // a = As + gi s
        ga[0] = __fmaf_rn(pr, br, pi * bi);     ga[1] = __fmaf_rn(pr, bi, -(pi * br));
        gb[0] = __fmaf_rn(pr, ar, -(pi * ai));  gb[1] = __fmaf_rn(pr, ai, pi * ar);
        gp[0] = __fmaf_rn(sr, br, si * bi) + __fmaf_rn(z, orr, z * oi);
        gp[1] = __fmaf_rn(sr, bi, -(si * br)) + __fmaf_rn(z, oi, -(z * orr));
    }
}

// NT: past the caches (the relation rows of the draws)
template <int W, bool NT>
__device__ __forceinline__ void rn_store(float* __restrict__ row, int c, const float (&v)[W]) {
    if constexpr (W == 4) {
        const f32x4 t = {v[0], v[1], v[2], v[3]};
        if constexpr (NT) __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(row + c));
        else *reinterpret_cast<f32x4*>(row + c) = t;
    } else {
        if constexpr (NT) __builtin_nontemporal_store(v[0], row + c);
        else row[c] = v[0];
    }
}

template <int MODEL, int W>
__global__ __launch_bounds__(kRnThreads) void relneg_backward_kernel(const RelnegParams P) {
    constexpr bool TWO = MODEL == EMG_COMPLEX || MODEL == EMG_HOLE || MODEL == EMG_ROTATE || MODEL == EMG_SIMPLE;   // rows of two halves
    constexpr bool NORM = MODEL == EMG_TRANSE_L2 || MODEL == EMG_TRANSE_P;
    constexpr int NV = TWO ? 2 : 1;
    const int64_t t = (int64_t)blockIdx.x * kRnThreads + threadIdx.x;
    const int64_t B = P.B;
    if (t >= B * P.nq) return;   // (no workgroup barrier below)
    const int64_t i = t / P.nq;
    const int c = (int)(t - i * P.nq) * W;
    const int n = TWO ? P.k_int >> 1 : P.k_int;   // the partner of column c is column n + c
    const int s = P.pos[3 * i], p = P.pos[3 * i + 1], o = P.pos[3 * i + 2];
    const float* srow = P.ent + (int64_t)s * P.ld_ent;
    const float* orow = P.ent + (int64_t)o * P.ld_ent;
    const int64_t roff = P.g_pos ? B : 0;   // the draws' relation rows start behind the positives' own
    const bool writes_dest = c == 0;

    float a[NV][W], b[NV][W];
#pragma unroll
    for (int v = 0; v < NV; ++v) { rn_load<W>(srow, v * n + c, a[v]); rn_load<W>(orow, v * n + c, b[v]); }
    double As[NV][W], Ao[NV][W];
    if (writes_dest) { P.dest_ent[i] = s; P.dest_ent[B + i] = o; }

    // one triple (s, pp, o) under dL/dscore g: its relation row to slot `slot`, its entity terms into the sums
    auto triple = [&](int pp, float g, float raw, int64_t slot, bool first, auto nt_tag) {
        constexpr bool NT = decltype(nt_tag)::value;
        const float* prow = P.rel + (int64_t)pp * P.ld_rel;
        float pr[NV][W];
        rn_load<W>(prow, c, pr[0]);
        if constexpr (TWO) {
            if constexpr (MODEL == EMG_ROTATE) {
#pragma unroll
                for (int w = 0; w < W; ++w) pr[1][w] = 0.f;   // the phase row has one half
            } else {
                rn_load<W>(prow, n + c, pr[1]);
            }
        }
        float nrm;
        const float gi = rn_coef<MODEL>(g, raw, P.scale, &nrm);
        float gr[NV][W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const float av[2] = {a[0][w], a[NV - 1][w]}, pv[2] = {pr[0][w], pr[NV - 1][w]}, bv[2] = {b[0][w], b[NV - 1][w]};
            float ga[2], gp[2], gb[2];
            rn_term<MODEL>(av, pv, bv, gi, nrm, P.scale, ga, gp, gb);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                gr[v][w] = gp[v];
                As[v][w] = first ? (double)ga[v] : As[v][w] + (double)ga[v];
                Ao[v][w] = first ? (double)gb[v] : Ao[v][w] + (double)gb[v];
            }
        }
        float* crow = P.contrib_rel + slot * P.ldc;
#pragma unroll
        for (int v = 0; v < NV; ++v) rn_store<W, NT>(crow, v * n + c, gr[v]);
        if (writes_dest) P.dest_rel[slot] = pp;
    };

    bool first = true;
    if (P.g_pos) {
        triple(p, P.g_pos[i], NORM ? P.raw_pos[i] : 0.f, i, true, std::false_type{});
        first = false;
    }
    for (int j = 0; j < P.eta; ++j) {
        const int64_t at = (int64_t)j * B + i;
        const int pp = relneg_shift(P.codes[at], p, P.n_rel);
        triple(pp, P.g_neg[at], NORM ? P.raw_neg[at] : 0.f, roff + at, first, std::true_type{});
        first = false;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        float fs[W], fo[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { fs[w] = (float)As[v][w]; fo[w] = (float)Ao[v][w]; }
        rn_store<W, false>(P.contrib_ent + i * P.ldc, v * n + c, fs);
        rn_store<W, false>(P.contrib_ent + (B + i) * P.ldc, v * n + c, fo);
    }
}

bool rn_two_halves(int model) { return model == EMG_COMPLEX || model == EMG_HOLE || model == EMG_ROTATE || model == EMG_SIMPLE; }

int relneg_check(const emg_relneg_args* a, const char* who, RelnegParams* P, bool* vec) {
    EMG_REQUIRE(a, "%s: null args", who);
    EMG_REQUIRE((a->model >= 0 && a->model <= EMG_ROTATE) || a->model == EMG_SIMPLE, "%s: unknown model %d", who, (int)a->model);
    EMG_REQUIRE(a->B >= 0 && a->eta >= 1, "%s: bad sizes (B = %lld, eta = %d)", who, (long long)a->B, (int)a->eta);
    EMG_REQUIRE(a->n_rel >= 2, "%s: n_rel = %lld: a relation negative needs another relation", who, (long long)a->n_rel);
    EMG_REQUIRE(a->n_rel < ((int64_t)1 << 31) && a->n_ent > 0 && a->n_ent < ((int64_t)1 << 31), "%s: bad table sizes", who);
    EMG_REQUIRE(a->k_int > 0 && a->ld_ent >= a->k_int && a->ld_rel >= a->k_int, "%s: bad strides", who);
    EMG_REQUIRE(!rn_two_halves(a->model) || a->k_int % 2 == 0, "%s: odd k_int for a model whose rows have two halves", who);
    EMG_REQUIRE(a->model != EMG_TRANSE_P || a->scale > 0.f, "%s: EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive", who);
    if (a->B == 0) return EMG_OK;
    EMG_REQUIRE(a->ent && a->rel && a->pos && a->codes, "%s: null pointer", who);
    P->model = a->model; P->k_int = a->k_int; P->scale = a->scale; P->eta = a->eta;
    P->ent = a->ent; P->ld_ent = a->ld_ent; P->rel = a->rel; P->n_rel = a->n_rel; P->ld_rel = a->ld_rel;
    P->pos = a->pos; P->B = a->B; P->codes = a->codes;
    P->scores_pos = a->scores_pos; P->scores_neg = a->scores_neg;
    P->g_pos = a->g_pos; P->g_neg = a->g_neg; P->raw_pos = a->raw_pos; P->raw_neg = a->raw_neg;
    P->contrib_ent = a->contrib_ent; P->contrib_rel = a->contrib_rel; P->ldc = a->ldc;
    P->dest_ent = a->dest_ent; P->dest_rel = a->dest_rel;
    P->n_items = P->npos = P->nsl = P->n_slices = P->nq = 0;
    // 16-byte row loads: rows 16-byte aligned, and groups of four columns that never straddle a row's end or a row's halves
    const int cols = rn_two_halves(a->model) ? a->k_int / 2 : a->k_int;
    *vec = cols % 4 == 0 && a->ld_ent % 4 == 0 && a->ld_rel % 4 == 0 && aligned16(a->ent) && aligned16(a->rel);
    return EMG_OK;
}

// waits for the launch and reports an idx the kernel refused
int relneg_flag(const char* who, hipStream_t st) {
    int32_t bad = 0;
    EMG_HIP(hipMemcpyFromSymbolAsync(&bad, HIP_SYMBOL(g_relneg_bad), sizeof(bad), 0, hipMemcpyDeviceToHost, st));
    EMG_HIP(hipStreamSynchronize(st));
    if (!bad) return EMG_OK;
    const int32_t zero = 0;
    EMG_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_relneg_bad), &zero, sizeof(zero), 0, hipMemcpyHostToDevice, st));
    EMG_HIP(hipStreamSynchronize(st));
    return fail(EMG_EINVAL, "%s: codes hold an idx outside [0, n_rel - 1)", who);
}

int rn_kind(int model) {
    switch (model) {
        case EMG_TRANSE_L1: return RK_L1;
        case EMG_TRANSE_L2: return RK_L2;
        case EMG_TRANSE_P: return RK_P;
        case EMG_DISTMULT: return RK_DOT;
        case EMG_ROTATE: return RK_ROT;
        case EMG_SIMPLE: return RK_SIMPLE;
        default: return RK_CPLX;
    }
}

template <bool VEC>
void (*rn_forward_kernel(int kind))(const RelnegParams) {
    switch (kind) {
        case RK_DOT: return relneg_forward_kernel<RK_DOT, VEC>;
        case RK_L1: return relneg_forward_kernel<RK_L1, VEC>;
        case RK_L2: return relneg_forward_kernel<RK_L2, VEC>;
        case RK_P: return relneg_forward_kernel<RK_P, VEC>;
        case RK_CPLX: return relneg_forward_kernel<RK_CPLX, VEC>;
        case RK_SIMPLE: return relneg_forward_kernel<RK_SIMPLE, VEC>;
        default: return relneg_forward_kernel<RK_ROT, VEC>;
    }
}

template <int W>
void (*rn_backward_kernel(int model))(const RelnegParams) {
    switch (model) {
        case EMG_TRANSE_L1: return relneg_backward_kernel<EMG_TRANSE_L1, W>;
        case EMG_TRANSE_L2: return relneg_backward_kernel<EMG_TRANSE_L2, W>;
        case EMG_DISTMULT: return relneg_backward_kernel<EMG_DISTMULT, W>;
        case EMG_COMPLEX: return relneg_backward_kernel<EMG_COMPLEX, W>;
        case EMG_HOLE: return relneg_backward_kernel<EMG_HOLE, W>;
        case EMG_TRANSE_P: return relneg_backward_kernel<EMG_TRANSE_P, W>;
        case EMG_SIMPLE: return relneg_backward_kernel<EMG_SIMPLE, W>;
        default: return relneg_backward_kernel<EMG_ROTATE, W>;
    }
}

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" int emg_relneg_forward(const emg_relneg_args* a, void* stream) {
    RelnegParams P;
    bool vec = false;
    const int rc = relneg_check(a, "emg_relneg_forward", &P, &vec);
    if (rc != EMG_OK || a->B == 0) return rc;
    EMG_REQUIRE(a->scores_neg, "emg_relneg_forward: null scores_neg");
    P.n_items = a->eta + (a->scores_pos ? 1 : 0);
    const int cap = kRnThreads * kRnItems;                      // chains of a workgroup
    P.nsl = P.n_items < cap ? P.n_items : cap;                  // items per slice: every positive of the run has the same
    P.n_slices = (int32_t)cdiv(P.n_items, P.nsl);
    P.npos = cap / P.nsl < kRnMaxPos ? cap / P.nsl : kRnMaxPos;
    const int64_t blocks = cdiv(a->B, P.npos) * P.n_slices;
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_relneg_forward: too many workgroups");
    hipStream_t st = (hipStream_t)stream;
    void (*fn)(const RelnegParams) = vec ? rn_forward_kernel<true>(rn_kind(a->model)) : rn_forward_kernel<false>(rn_kind(a->model));
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kRnThreads), 0, st, P);
    EMG_LAUNCH_CHECK();
    return relneg_flag("emg_relneg_forward", st);
}

extern "C" int emg_relneg_backward(const emg_relneg_args* a, void* stream) {
    RelnegParams P;
    bool vec = false;
    const int rc = relneg_check(a, "emg_relneg_backward", &P, &vec);
    if (rc != EMG_OK || a->B == 0) return rc;
    EMG_REQUIRE(a->g_neg && a->contrib_ent && a->contrib_rel && a->dest_ent && a->dest_rel, "emg_relneg_backward: null pointer");
    EMG_REQUIRE(a->ldc >= a->k_int, "emg_relneg_backward: ldc < k_int");
    const bool norm = a->model == EMG_TRANSE_L2 || a->model == EMG_TRANSE_P;
    EMG_REQUIRE(!norm || (a->raw_neg && (a->raw_pos || !a->g_pos)),
                "emg_relneg_backward: TransE-L2 / TransE-p need the raw scores (raw_neg, and raw_pos with g_pos)");
    if (a->model == EMG_TRANSE_P && std::isinf(a->scale))
        return fail(EMG_ENOSUP, "emg_relneg_backward: EMG_TRANSE_P of infinite order is not available with relation negatives");
    vec = vec && a->ldc % 4 == 0 && aligned16(a->contrib_ent) && aligned16(a->contrib_rel);   // 16-byte row stores too
    const int cols = rn_two_halves(a->model) ? a->k_int / 2 : a->k_int;
    P.nq = vec ? cols / 4 : cols;
    const int64_t blocks = cdiv(a->B * P.nq, kRnThreads);
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_relneg_backward: too many workgroups");
    hipStream_t st = (hipStream_t)stream;
    void (*fn)(const RelnegParams) = vec ? rn_backward_kernel<4>(a->model) : rn_backward_kernel<1>(a->model);
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kRnThreads), 0, st, P);
    EMG_LAUNCH_CHECK();
    return relneg_flag("emg_relneg_backward", st);
}
