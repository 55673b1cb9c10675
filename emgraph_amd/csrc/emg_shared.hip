// emg_shared.hip — shared negatives: chunks of C consecutive positives scored against common draws (DESIGN.md 0 A-26, 4.1
// "Shared negatives"; include/emgraph_hip.h has the contract).
//
// The ordinary step gathers 2 + eta_total entity rows per positive and writes as many gradient rows; here a chunk of C positives
// shares its eta_total replacement rows, so the gather per positive is 2 + eta_total / C rows and the step writes 2 B + eta_total * G
// gradient rows (G = ceil(B / C)).  Arithmetic is the ordinary step's (every positive still meets eta_total negatives) and is small
// against the bytes; both kernels are VALU tiles over rows staged in LDS, in column blocks (a chunk's rows do not fit LDS whole):
//   forward   a workgroup = (chunk, slice of the chunk's draws).  Per column block it builds the C object-side and C subject-side
//             query rows (the formulas of emg_rank.hip::build_queries_kernel) and copies the slice's replacement rows into LDS;
//             a thread carries up to kShPairs (positive, draw) accumulators through the blocks, k ascending: the canonical chain
//             of emg_chain.hpp, so a score has the bits emg_eval_scores_dense gives for the same (query row, candidate).
//   backward  a workgroup = (chunk, column block): a gradient column depends on that column of the rows and on per-pair scalars
//             only.  It stages the raw s / p / o rows and ALL replacement rows of the chunk for its block, then
//               phase A  one thread per (positive, column): the positive's own term, then the draws in ascending m -> dE[s], dE[o], dR[p]
//               phase B  one thread per (draw, column): the chunk's positives in ascending i                        -> dE[replacement]
//             Fixed orders, no atomics: two runs give the same bits.  A term is the f32 product the ordinary step stores as a
//             gradient row; the sums over terms are carried in double and rounded once (the arithmetic is free here).  Block 0
//             of a chunk also writes the destinations.
#include <cmath>

#include "emg_chain.hpp"

// explicit operations only (the canonical chain; emg_chain.hpp sets the same)
#pragma clang fp contract(off)

namespace emg {

constexpr int kShThreads = 256;
constexpr int kShPairs = 8;            // (positive, draw) pairs a forward thread carries
constexpr int kShLdsBytes = 60000;     // dynamic LDS a launch may ask for without opting in to more

struct SharedParams {
    int32_t model, k_int; float scale; int32_t eta_total;
    const float* ent; int64_t ld_ent; const float* rel; int64_t ld_rel;
    const int32_t* pos; int64_t B; int32_t C; int64_t G; const int32_t* codes;
    float* scores_pos; float* scores_neg;
    const float* g_pos; const float* g_neg; const float* raw_pos; const float* raw_neg;
    float* contrib_ent; float* contrib_rel; int64_t ldc; int32_t* dest_ent; int32_t* dest_rel;
    int32_t kb;         // LDS columns per block (pair layout: kb / 2 complex coordinates, re in [0, kb/2), im in [kb/2, kb))
    int32_t nsl;        // forward: draws per slice
    int32_t n_slices;   // forward: slices per chunk
    int32_t n_cb;       // column blocks
};

__host__ __device__ __forceinline__ bool sh_is_complex(int model) { return model == EMG_COMPLEX || model == EMG_HOLE || model == EMG_ROTATE; }

// global column of LDS column lc of block b, -1 past the row's end.  PAIR: the block holds complex coordinates [b h, b h + h), h = kb / 2
template <bool PAIR>
__device__ __forceinline__ int sh_gcol(int b, int kb, int k_int, int lc) {
    if constexpr (PAIR) {
        const int h = kb >> 1, n = k_int >> 1;
        const int j = b * h + (lc < h ? lc : lc - h);
        if (j >= n) return -1;
        return lc < h ? j : n + j;
    } else {
        const int c = b * kb + lc;
        return c < k_int ? c : -1;
    }
}

template <int W>
__device__ __forceinline__ void sh_load(const float* __restrict__ row, int gc, float (&v)[W]) {
    if constexpr (W == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(row + gc);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = row[gc];
    }
}

// one element of the two query rows of (s, p, o): emg_rank.hip::build_queries_kernel's expressions.  Real models read the *_r values
// only; complex models: hi = the column lies in the imaginary half; RotatE: p_r is the phase
__device__ __forceinline__ void sh_query_elem(int model, bool hi, float s_r, float s_i, float p_r, float p_i, float o_r, float o_i,
                                              float* qo, float* qs) {
    if (model == EMG_TRANSE_L1 || model == EMG_TRANSE_L2 || model == EMG_TRANSE_P) {
        *qo = __fadd_rn(s_r, p_r);
        *qs = __fsub_rn(o_r, p_r);
    } else if (model == EMG_DISTMULT) {
        *qo = __fmul_rn(p_r, s_r);
        *qs = __fmul_rn(p_r, o_r);
    } else {
        if (model == EMG_ROTATE) {
            const float th = p_r;
            sincosf(th, &p_i, &p_r);
        }
        if (!hi) {
            *qo = __fmaf_rn(p_r, s_r, -__fmul_rn(p_i, s_i));
            *qs = __fmaf_rn(p_r, o_r, __fmul_rn(p_i, o_i));
        } else {
            *qo = __fmaf_rn(p_r, s_i, __fmul_rn(p_i, s_r));
            *qs = __fmaf_rn(p_r, o_i, -__fmul_rn(p_i, o_r));
        }
    }
}

// KIND: 0 dot models, 1 TransE-L1, 2 TransE-L2, 3 TransE-p, 4 RotatE (PAIR layout)
template <int KIND>
__device__ __forceinline__ float sh_final(int model, float acc, float scale) {
    if constexpr (KIND == 0) return model == EMG_HOLE ? __fmul_rn(acc, scale) : acc;
    else if constexpr (KIND == 2) return -sqrtf(acc);
    else if constexpr (KIND == 3) return isinf(scale) ? -acc : -powf(acc, 1.0f / scale);
    else return -acc;
}

template <int KIND>
__device__ __forceinline__ float sh_step(float q, float e, float acc, float scale) {
    if constexpr (KIND == 3) {
        const float ad = fabsf(__fsub_rn(q, e));
        return isinf(scale) ? fmaxf(acc, ad) : __fadd_rn(acc, powf(ad, scale));
    } else {
        return chain_step<KIND>(q, e, acc);
    }
}

// LDS of the forward: q_o [C][ldl] | q_s [C][ldl] | e [nsl][ldl] | ids int [3 C] | codes int [nsl];  ldl = kb + 1 (odd: threads of
// a wave that walk consecutive positives hit distinct banks)
template <int KIND, bool VEC>
__global__ __launch_bounds__(kShThreads) void shared_forward_kernel(const SharedParams P) {
    extern __shared__ float sh_lds[];
    constexpr bool PAIR = KIND == 4;
    constexpr int W = VEC ? 4 : 1;
    const int tid = threadIdx.x;
    const int C = P.C, kb = P.kb, ldl = kb + 1, k_int = P.k_int, n = k_int >> 1;
    const int64_t g = blockIdx.x / P.n_slices;
    const int sl = (int)(blockIdx.x - g * P.n_slices);
    const int64_t i0 = g * C;
    const int Cn = (int)(P.B - i0 < C ? P.B - i0 : C);
    const int m0 = sl * P.nsl;
    const int nm = P.eta_total - m0 < P.nsl ? P.eta_total - m0 : P.nsl;
    float* q_o = sh_lds;
    float* q_s = q_o + C * ldl;
    float* e_s = q_s + C * ldl;
    int* ids = reinterpret_cast<int*>(e_s + P.nsl * ldl);
    int* cd = ids + 3 * C;
    const bool cplx = sh_is_complex(P.model);

    for (int t = tid; t < Cn; t += kShThreads) {
        ids[t] = P.pos[3 * (i0 + t)];
        ids[C + t] = P.pos[3 * (i0 + t) + 1];
        ids[2 * C + t] = P.pos[3 * (i0 + t) + 2];
    }
    for (int t = tid; t < nm; t += kShThreads) cd[t] = P.codes[(int64_t)(m0 + t) * P.G + g];
    __syncthreads();

    float acc[kShPairs];
    int qoff[kShPairs], eoff[kShPairs];
    bool act[kShPairs];
#pragma unroll
    for (int r = 0; r < kShPairs; ++r) {
        const int pp = tid + kShThreads * r;
        const int ml = pp / C, i = pp - ml * C;
        act[r] = i < Cn && ml < nm;
        acc[r] = 0.f;
        qoff[r] = 0; eoff[r] = 0;
        if (act[r]) {
            qoff[r] = (cd[ml] < 0 ? 0 : C * ldl) + i * ldl;   // keep_subject: the object is replaced -> object-side query
            eoff[r] = ml * ldl;
        }
    }
    const bool do_pos = sl == 0 && tid < Cn;
    const float* o_row = P.ent + (do_pos ? (int64_t)ids[2 * C + tid] * P.ld_ent : 0);
    float acc_pos = 0.f;

    const int gw = kb / W;   // load groups per LDS row
    for (int b = 0; b < P.n_cb; ++b) {
        // the two query rows of every positive of the chunk
        for (int it = tid; it < Cn * gw; it += kShThreads) {
            const int i = it / gw, lc0 = (it - i * gw) * W;
            const int gc0 = sh_gcol<PAIR>(b, kb, k_int, lc0);
            if (gc0 < 0) continue;
            const float* s = P.ent + (int64_t)ids[i] * P.ld_ent;
            const float* p = P.rel + (int64_t)ids[C + i] * P.ld_rel;
            const float* o = P.ent + (int64_t)ids[2 * C + i] * P.ld_ent;
            float sr[W], si[W], pr[W], pi[W], orr[W], oi[W];
            bool hi = false;
            if (cplx) {
                hi = gc0 >= n;
                const int cj = hi ? gc0 - n : gc0;
                sh_load<W>(s, cj, sr); sh_load<W>(s, n + cj, si);
                sh_load<W>(p, cj, pr);
                if (P.model != EMG_ROTATE) sh_load<W>(p, n + cj, pi);
                sh_load<W>(o, cj, orr); sh_load<W>(o, n + cj, oi);
            } else {
                sh_load<W>(s, gc0, sr); sh_load<W>(p, gc0, pr); sh_load<W>(o, gc0, orr);
            }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                float qo, qs;
                sh_query_elem(P.model, hi, sr[w], cplx ? si[w] : 0.f, pr[w], (cplx && P.model != EMG_ROTATE) ? pi[w] : 0.f, orr[w],
                              cplx ? oi[w] : 0.f, &qo, &qs);
                q_o[i * ldl + lc0 + w] = qo;
                q_s[i * ldl + lc0 + w] = qs;
            }
        }
        // the slice's replacement rows
        for (int it = tid; it < nm * gw; it += kShThreads) {
            const int ml = it / gw, lc0 = (it - ml * gw) * W;
            const int gc0 = sh_gcol<PAIR>(b, kb, k_int, lc0);
            if (gc0 < 0) continue;
            float v[W];
            sh_load<W>(P.ent + (int64_t)(cd[ml] & 0x7fffffff) * P.ld_ent, gc0, v);
#pragma unroll
            for (int w = 0; w < W; ++w) e_s[ml * ldl + lc0 + w] = v[w];
        }
        __syncthreads();
        if constexpr (PAIR) {
            const int h = kb >> 1;
            const int jv = n - b * h < h ? n - b * h : h;
            for (int jj = 0; jj < jv; ++jj) {
#pragma unroll
                for (int r = 0; r < kShPairs; ++r)
                    acc[r] = rotate_step(q_o[qoff[r] + jj], q_o[qoff[r] + h + jj], e_s[eoff[r] + jj], e_s[eoff[r] + h + jj], acc[r]);
                if (do_pos) acc_pos = rotate_step(q_o[tid * ldl + jj], q_o[tid * ldl + h + jj], o_row[b * h + jj], o_row[n + b * h + jj], acc_pos);
            }
        } else {
            const int kv = k_int - b * kb < kb ? k_int - b * kb : kb;
            for (int cc = 0; cc < kv; ++cc) {
#pragma unroll
                for (int r = 0; r < kShPairs; ++r) acc[r] = sh_step<KIND>(q_o[qoff[r] + cc], e_s[eoff[r] + cc], acc[r], P.scale);
                if (do_pos) acc_pos = sh_step<KIND>(q_o[tid * ldl + cc], o_row[b * kb + cc], acc_pos, P.scale);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kShPairs; ++r) {
        if (!act[r]) continue;
        const int pp = tid + kShThreads * r;
        const int ml = pp / C, i = pp - ml * C;
        P.scores_neg[(int64_t)(m0 + ml) * P.B + i0 + i] = sh_final<KIND>(P.model, acc[r], P.scale);
    }
    if (do_pos) P.scores_pos[i0 + tid] = sh_final<KIND>(P.model, acc_pos, P.scale);
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// gradient of one column (complex models: one coordinate, [re, im]) of the triple (a, p, b) under the upstream coefficient gi:
// the formulas of emg_train_backward_ex(fused_loss = -1) (emg_score_kernels.hpp::accum_grads, emg_score.hip's generic kernels).
//   gi   dL/dscore, for TransE-L2 already divided by the norm, for HolE already times the scale
//   nrm  TransE-p only: the triple's norm;  RotatE: p = (cos, sin) of the phase
template <int MODEL>
__device__ __forceinline__ void sh_grads(const float (&a)[2], const float (&p)[2], const float (&b)[2], float gi, float nrm, float ord,
                                         float (&ga)[2], float (&gp)[2], float (&gb)[2]) {
    if constexpr (MODEL == EMG_TRANSE_L1 || MODEL == EMG_TRANSE_L2) {
        const float d = (a[0] + p[0]) - b[0];
        const float t = MODEL == EMG_TRANSE_L1 ? gi * sgnf(d) : gi * d;
        ga[0] = -t; gp[0] = -t; gb[0] = t;
    } else if constexpr (MODEL == EMG_TRANSE_P) {
        const float d = (a[0] + p[0]) - b[0];
        const float ad = fabsf(d);
        float u = 0.f;
        if (nrm != 0.f && ad != 0.f) u = (d > 0.f ? 1.f : -1.f) * powf(ad, ord - 1.f) / powf(nrm, ord - 1.f);
        const float v = gi * u;
        ga[0] = -v; gp[0] = -v; gb[0] = v;
    } else if constexpr (MODEL == EMG_DISTMULT) {
        ga[0] = gi * (p[0] * b[0]);
        gp[0] = gi * (a[0] * b[0]);
        gb[0] = gi * (a[0] * p[0]);
    } else if constexpr (MODEL == EMG_ROTATE) {
        const float cn = p[0], sn = p[1];
        const float wr = __fmaf_rn(a[0], cn, -__fmul_rn(a[1], sn));
        const float wi = __fmaf_rn(a[0], sn, __fmul_rn(a[1], cn));
        const float dr = __fsub_rn(wr, b[0]), di = __fsub_rn(wi, b[1]);
        const float m = sqrtf(__fmaf_rn(dr, dr, __fmul_rn(di, di)));
        const float ur = m > 0.f ? dr / m : 0.f, ui = m > 0.f ? di / m : 0.f;
        ga[0] = -gi * (ur * cn + ui * sn); ga[1] = -gi * (ui * cn - ur * sn);
        gb[0] = gi * ur; gb[1] = gi * ui;
        gp[0] = gi * (ur * wi - ui * wr); gp[1] = 0.f;
    } else {   // ComplEx / HolE
        const float sr = a[0], si = a[1], pr = p[0], pi = p[1], orr = b[0], oi = b[1];
        ga[0] = gi * __fmaf_rn(pr, orr, pi * oi);    ga[1] = gi * __fmaf_rn(pr, oi, -(pi * orr));
        gp[0] = gi * __fmaf_rn(sr, orr, si * oi);    gp[1] = gi * __fmaf_rn(sr, oi, -(si * orr));
        gb[0] = gi * __fmaf_rn(pr, sr, -(pi * si));  gb[1] = gi * __fmaf_rn(pr, si, pi * sr);
    }
}

// the upstream coefficient sh_grads takes, from dL/dscore and the triple's raw score
template <int MODEL>
__device__ __forceinline__ float sh_coef(float g, float raw, float scale, float* nrm) {
    *nrm = 0.f;
    if constexpr (MODEL == EMG_TRANSE_L2) { const float nr = -raw; return nr > 0.f ? g / nr : 0.f; }
    else if constexpr (MODEL == EMG_TRANSE_P) { *nrm = -raw; return g; }
    else if constexpr (MODEL == EMG_HOLE) return g * scale;
    else return g;
}

// LDS of the backward: s [C][ldl] | p [C][ldl] | o [C][ldl] | e [eta_total][ldl] | ids int [3 C] | codes int [eta_total]
template <int MODEL, bool VEC>
__global__ __launch_bounds__(kShThreads) void shared_backward_kernel(const SharedParams P) {
    extern __shared__ float sh_lds[];
    constexpr bool PAIR = MODEL == EMG_COMPLEX || MODEL == EMG_HOLE || MODEL == EMG_ROTATE;
    constexpr bool NORM = MODEL == EMG_TRANSE_L2 || MODEL == EMG_TRANSE_P;
    constexpr int NV = PAIR ? 2 : 1;
    constexpr int W = VEC ? 4 : 1;
    const int tid = threadIdx.x;
    const int C = P.C, kb = P.kb, ldl = kb + 1, k_int = P.k_int, n = k_int >> 1, h = kb >> 1, et = P.eta_total;
    const int64_t g = blockIdx.x / P.n_cb;
    const int b = (int)(blockIdx.x - g * P.n_cb);
    const int64_t i0 = g * C, B = P.B;
    const int Cn = (int)(B - i0 < C ? B - i0 : C);
    float* s_s = sh_lds;
    float* p_s = s_s + C * ldl;
    float* o_s = p_s + C * ldl;
    float* e_s = o_s + C * ldl;
    int* ids = reinterpret_cast<int*>(e_s + et * ldl);
    int* cd = ids + 3 * C;

    for (int t = tid; t < Cn; t += kShThreads) {
        ids[t] = P.pos[3 * (i0 + t)];
        ids[C + t] = P.pos[3 * (i0 + t) + 1];
        ids[2 * C + t] = P.pos[3 * (i0 + t) + 2];
    }
    for (int t = tid; t < et; t += kShThreads) cd[t] = P.codes[(int64_t)t * P.G + g];
    __syncthreads();

    if (b == 0) {   // destinations of the chunk's gradient rows
        for (int t = tid; t < Cn; t += kShThreads) {
            P.dest_ent[i0 + t] = ids[t];
            P.dest_ent[B + i0 + t] = ids[2 * C + t];
            P.dest_rel[i0 + t] = ids[C + t];
        }
        for (int t = tid; t < et; t += kShThreads) P.dest_ent[2 * B + (int64_t)t * P.G + g] = cd[t] & 0x7fffffff;
    }

    const int gw = kb / W;
    for (int it = tid; it < (3 * Cn + et) * gw; it += kShThreads) {
        const int row = it / gw, lc0 = (it - row * gw) * W;
        const int gc0 = sh_gcol<PAIR>(b, kb, k_int, lc0);
        if (gc0 < 0) continue;
        const float* src;
        float* dst;
        bool phase = false;
        if (row < Cn) { src = P.ent + (int64_t)ids[row] * P.ld_ent; dst = s_s + row * ldl; }
        else if (row < 2 * Cn) { src = P.rel + (int64_t)ids[C + row - Cn] * P.ld_rel; dst = p_s + (row - Cn) * ldl; phase = MODEL == EMG_ROTATE; }
        else if (row < 3 * Cn) { src = P.ent + (int64_t)ids[2 * C + row - 2 * Cn] * P.ld_ent; dst = o_s + (row - 2 * Cn) * ldl; }
        else { src = P.ent + (int64_t)(cd[row - 3 * Cn] & 0x7fffffff) * P.ld_ent; dst = e_s + (row - 3 * Cn) * ldl; }
        float v[W];
        if (phase) {   // RotatE: the relation row holds phases in columns [0, n): stage cos in the re half, sin in the im half
            const bool hi = gc0 >= n;
            sh_load<W>(src, hi ? gc0 - n : gc0, v);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                float sn, cs;
                sincosf(v[w], &sn, &cs);
                v[w] = hi ? sn : cs;
            }
        } else {
            sh_load<W>(src, gc0, v);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) dst[lc0 + w] = v[w];
    }
    __syncthreads();

    // valid items (columns / coordinates) of this block, and the global column of item jj (second value of a pair: + n)
    const int nj = PAIR ? (n - b * h < h ? n - b * h : h) : (k_int - b * kb < kb ? k_int - b * kb : kb);
    const int gbase = PAIR ? b * h : b * kb;
    const int im = PAIR ? h : 0;   // LDS offset of a pair's second value

    // phase A: the positives' rows
    for (int it = tid; it < Cn * nj; it += kShThreads) {
        const int i = it / nj, jj = it - i * nj;
        const float s[2] = {s_s[i * ldl + jj], s_s[i * ldl + jj + im]};
        const float p[2] = {p_s[i * ldl + jj], p_s[i * ldl + jj + im]};
        const float o[2] = {o_s[i * ldl + jj], o_s[i * ldl + jj + im]};
        float ga[2], gp[2], gb[2], nrm;
        const float gi = sh_coef<MODEL>(P.g_pos[i0 + i], NORM ? P.raw_pos[i0 + i] : 0.f, P.scale, &nrm);
        sh_grads<MODEL>(s, p, o, gi, nrm, P.scale, ga, gp, gb);
        // the terms are the f32 products the ordinary step writes as rows; their SUM is kept in double and rounded once
        double As[2] = {ga[0], ga[1]}, Ap[2] = {gp[0], gp[1]}, Ao[2] = {gb[0], gb[1]};
        for (int m = 0; m < et; ++m) {
            const int64_t at = (int64_t)m * B + i0 + i;
            const float e[2] = {e_s[m * ldl + jj], e_s[m * ldl + jj + im]};
            const float gm = sh_coef<MODEL>(P.g_neg[at], NORM ? P.raw_neg[at] : 0.f, P.scale, &nrm);
            if (cd[m] < 0) {   // subject kept: (s, p, e)
                sh_grads<MODEL>(s, p, e, gm, nrm, P.scale, ga, gp, gb);
#pragma unroll
                for (int v = 0; v < NV; ++v) { As[v] += ga[v]; Ap[v] += gp[v]; }
            } else {           // object kept: (e, p, o)
                sh_grads<MODEL>(e, p, o, gm, nrm, P.scale, ga, gp, gb);
#pragma unroll
                for (int v = 0; v < NV; ++v) { Ao[v] += gb[v]; Ap[v] += gp[v]; }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int gc = gbase + jj + v * n;
            P.contrib_ent[(i0 + i) * P.ldc + gc] = (float)As[v];
            P.contrib_ent[(B + i0 + i) * P.ldc + gc] = (float)Ao[v];
            P.contrib_rel[(i0 + i) * P.ldc + gc] = (float)Ap[v];
        }
    }

    // phase B: the shared rows
    for (int it = tid; it < et * nj; it += kShThreads) {
        const int m = it / nj, jj = it - m * nj;
        const float e[2] = {e_s[m * ldl + jj], e_s[m * ldl + jj + im]};
        const bool keep = cd[m] < 0;
        double Ae[2] = {0.0, 0.0};
        for (int i = 0; i < Cn; ++i) {
            const int64_t at = (int64_t)m * B + i0 + i;
            const float s[2] = {s_s[i * ldl + jj], s_s[i * ldl + jj + im]};
            const float p[2] = {p_s[i * ldl + jj], p_s[i * ldl + jj + im]};
            const float o[2] = {o_s[i * ldl + jj], o_s[i * ldl + jj + im]};
            float nrm;
            const float gm = sh_coef<MODEL>(P.g_neg[at], NORM ? P.raw_neg[at] : 0.f, P.scale, &nrm);
            float ga[2], gp[2], gb[2];
            if (keep) {
                sh_grads<MODEL>(s, p, e, gm, nrm, P.scale, ga, gp, gb);
#pragma unroll
                for (int v = 0; v < NV; ++v) Ae[v] += gb[v];
            } else {
                sh_grads<MODEL>(e, p, o, gm, nrm, P.scale, ga, gp, gb);
#pragma unroll
                for (int v = 0; v < NV; ++v) Ae[v] += ga[v];
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) P.contrib_ent[(2 * B + (int64_t)m * P.G + g) * P.ldc + gbase + jj + v * n] = (float)Ae[v];
    }
}

static int shared_check(const emg_shared_args* a, const char* who, SharedParams* P, bool* vec) {
    EMG_REQUIRE(a, "%s: null args", who);
    EMG_REQUIRE(a->model >= 0 && a->model <= EMG_ROTATE, "%s: unknown model %d", who, (int)a->model);
    EMG_REQUIRE(a->C >= 1 && a->C <= 256, "%s: C = %d outside [1, 256]", who, (int)a->C);
    EMG_REQUIRE(a->B >= 0 && a->eta_total >= 1, "%s: bad sizes (B = %lld, eta_total = %d)", who, (long long)a->B, (int)a->eta_total);
    EMG_REQUIRE(a->k_int > 0 && a->ld_ent >= a->k_int && a->ld_rel >= a->k_int, "%s: bad strides", who);
    EMG_REQUIRE(!sh_is_complex(a->model) || a->k_int % 2 == 0, "%s: odd k_int for a complex model", who);
    EMG_REQUIRE(a->model != EMG_TRANSE_P || a->scale > 0.f, "%s: EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive", who);
    EMG_REQUIRE(a->n_ent > 0 && a->n_ent < ((int64_t)1 << 31) && a->n_rel > 0, "%s: bad table sizes", who);
    if (a->B == 0) return EMG_OK;
    EMG_REQUIRE(a->ent && a->rel && a->pos && a->chunk_codes, "%s: null pointer", who);
    P->model = a->model; P->k_int = a->k_int; P->scale = a->scale; P->eta_total = a->eta_total;
    P->ent = a->ent; P->ld_ent = a->ld_ent; P->rel = a->rel; P->ld_rel = a->ld_rel;
    P->pos = a->pos; P->B = a->B; P->C = a->C; P->G = cdiv(a->B, a->C); P->codes = a->chunk_codes;
    P->scores_pos = a->scores_pos; P->scores_neg = a->scores_neg;
    P->g_pos = a->g_pos; P->g_neg = a->g_neg; P->raw_pos = a->raw_pos; P->raw_neg = a->raw_neg;
    P->contrib_ent = a->contrib_ent; P->contrib_rel = a->contrib_rel; P->ldc = a->ldc;
    P->dest_ent = a->dest_ent; P->dest_rel = a->dest_rel;
    P->kb = P->nsl = P->n_slices = P->n_cb = 0;
    // 16-byte row loads: rows 16-byte aligned, and groups of four columns that never straddle a row's end or a complex row's halves
    const int cols = sh_is_complex(a->model) ? a->k_int / 2 : a->k_int;
    *vec = cols % 4 == 0 && a->ld_ent % 4 == 0 && a->ld_rel % 4 == 0 && ((uintptr_t)a->ent & 15) == 0 && ((uintptr_t)a->rel & 15) == 0;
    return EMG_OK;
}

}  // namespace emg

using namespace emg;

extern "C" int emg_shared_forward(const emg_shared_args* a, void* stream) {
    SharedParams P;
    bool vec = false;
    const int rc = shared_check(a, "emg_shared_forward", &P, &vec);
    if (rc != EMG_OK || a->B == 0) return rc;
    EMG_REQUIRE(a->scores_pos && a->scores_neg, "emg_shared_forward: null scores");
    int cap = kShThreads * kShPairs / a->C;                      // draws per slice: at most kShPairs pairs per thread,
    if (cap > 256) cap = 256;                                    // and no more rows than a small chunk's LDS holds at full width
    P.n_slices = (int32_t)cdiv(a->eta_total, cap);
    // (no more slices than the accumulators ask for: every slice builds the chunk's 2 C query rows again, and that is what the
    // kernel spends its time on — C3 shape, C = 64: one slice per chunk 0.124 ms, three 0.169 ms)
    P.nsl = (int32_t)cdiv(a->eta_total, P.n_slices);
    const bool pair = a->model == EMG_ROTATE;
    size_t bytes = 0;
    for (int kb = 32; kb >= 8; kb >>= 1) {
        bytes = (size_t)(2 * a->C + P.nsl) * (kb + 1) * 4 + (size_t)(3 * a->C + P.nsl) * 4;
        if (bytes <= (size_t)kShLdsBytes) { P.kb = kb; break; }
    }
    EMG_REQUIRE(P.kb > 0, "emg_shared_forward: the chunk does not fit a workgroup's LDS");
    P.n_cb = (int32_t)(pair ? cdiv(a->k_int / 2, P.kb / 2) : cdiv(a->k_int, P.kb));
    const int64_t blocks = P.G * P.n_slices;
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_shared_forward: too many workgroups");
    const dim3 grid((unsigned)blocks), block(kShThreads);
    hipStream_t st = (hipStream_t)stream;
#define EMG_SH_FWD(KIND)                                                                                              \
    do {                                                                                                              \
        if (vec) hipLaunchKernelGGL((shared_forward_kernel<KIND, true>), grid, block, bytes, st, P);                  \
        else hipLaunchKernelGGL((shared_forward_kernel<KIND, false>), grid, block, bytes, st, P);                     \
    } while (0)
    switch (a->model) {
        case EMG_TRANSE_L1: EMG_SH_FWD(1); break;
        case EMG_TRANSE_L2: EMG_SH_FWD(2); break;
        case EMG_TRANSE_P: EMG_SH_FWD(3); break;
        case EMG_ROTATE: EMG_SH_FWD(4); break;
        default: EMG_SH_FWD(0); break;
    }
#undef EMG_SH_FWD
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_shared_backward(const emg_shared_args* a, void* stream) {
    SharedParams P;
    bool vec = false;
    const int rc = shared_check(a, "emg_shared_backward", &P, &vec);
    if (rc != EMG_OK || a->B == 0) return rc;
    EMG_REQUIRE(a->g_pos && a->g_neg && a->contrib_ent && a->contrib_rel && a->dest_ent && a->dest_rel, "emg_shared_backward: null pointer");
    EMG_REQUIRE(a->ldc >= a->k_int, "emg_shared_backward: ldc < k_int");
    const bool norm = a->model == EMG_TRANSE_L2 || a->model == EMG_TRANSE_P;
    EMG_REQUIRE(!norm || (a->raw_pos && a->raw_neg), "emg_shared_backward: TransE-L2 / TransE-p need the raw scores (raw_pos, raw_neg)");
    if (a->model == EMG_TRANSE_P && std::isinf(a->scale))
        return fail(EMG_ENOSUP, "emg_shared_backward: EMG_TRANSE_P of infinite order is not available with shared negatives");
    const bool pair = sh_is_complex(a->model);
    const int64_t rows = 3 * (int64_t)a->C + a->eta_total;
    size_t bytes = 0;
    for (int kb = 32; kb >= 8; kb >>= 1) {
        bytes = (size_t)rows * (kb + 1) * 4 + (size_t)rows * 4;
        if (bytes <= (size_t)kShLdsBytes) { P.kb = kb; break; }
    }
    EMG_REQUIRE(P.kb > 0, "emg_shared_backward: 3 C + eta_total = %lld rows do not fit a workgroup's LDS (at most 1500)", (long long)rows);
    P.n_cb = (int32_t)(pair ? cdiv(a->k_int / 2, P.kb / 2) : cdiv(a->k_int, P.kb));
    const int64_t blocks = P.G * P.n_cb;
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_shared_backward: too many workgroups");
    const dim3 grid((unsigned)blocks), block(kShThreads);
    hipStream_t st = (hipStream_t)stream;
#define EMG_SH_BWD(M)                                                                                                 \
    case M:                                                                                                           \
        if (vec) hipLaunchKernelGGL((shared_backward_kernel<M, true>), grid, block, bytes, st, P);                    \
        else hipLaunchKernelGGL((shared_backward_kernel<M, false>), grid, block, bytes, st, P);                       \
        break
    switch (a->model) {
        EMG_SH_BWD(EMG_TRANSE_L1);
        EMG_SH_BWD(EMG_TRANSE_L2);
        EMG_SH_BWD(EMG_DISTMULT);
        EMG_SH_BWD(EMG_COMPLEX);
        EMG_SH_BWD(EMG_HOLE);
        EMG_SH_BWD(EMG_TRANSE_P);
        default:
            if (vec) hipLaunchKernelGGL((shared_backward_kernel<EMG_ROTATE, true>), grid, block, bytes, st, P);
            else hipLaunchKernelGGL((shared_backward_kernel<EMG_ROTATE, false>), grid, block, bytes, st, P);
            break;
    }
#undef EMG_SH_BWD
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
