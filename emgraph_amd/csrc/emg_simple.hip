// emg_simple.hip — SimplE (EMG_SIMPLE; include/emgraph_hip.h has the contract): the kernels that look at (s, p, o)
// rows themselves.  Ranking needs none: a SimplE query row runs the scaled contraction chain of the tiled kernels (emg_common.hpp:
// chain_model); the query builder's branch is in emg_rank.hip, the relation-side kind in emg_relrank.hip.
//
// Rows are [h | t] (entities) and [r | r_inv] (relations), k = k_int / 2 columns per half; with swap(x) exchanging the halves
//   f(s, p, o) = scale * sum_{c < 2k} e_s[c] rel_p[c] swap(e_o)[c]
// Generic kernels of the shape of EMG_TRANSE_P's and EMG_ROTATE's (emg_score.hip): a wave per triple (inference) or per positive
// group (training: the positive and its eta negatives), any width, any row stride and alignment, rows read through the caches.
// Lane l owns columns l, l + 64, ... of BOTH halves: every row is read as two streams of consecutive floats across the wave, and the
// half-swapped partner of a column the lane owns is a column of the other stream at the same lane.  Summation order is fixed — a
// lane's columns ascending (first half, then second half, of each j), then the xor butterfly — every product and sum is an explicit
// correctly rounded operation, nothing is atomic: two runs give the same bits.
#include "emg_common.hpp"

#pragma clang fp contract(off)

namespace emg {
namespace {

__device__ __forceinline__ float simple_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off, 64));
    return v;
}

// the score of the triple (a, r, b): the one routine of emg_score_triples, the forward's positive and its negatives (all 64 lanes;
// the same value in every lane)
__device__ __forceinline__ float simple_score(const float* __restrict__ a, const float* __restrict__ r, const float* __restrict__ b,
                                              int half, float scale, int lane) {
    float acc = 0.f;
    for (int j = lane; j < half; j += 64) {
        acc = __fmaf_rn(__fmul_rn(a[j], r[j]), b[half + j], acc);
        acc = __fmaf_rn(__fmul_rn(a[half + j], r[half + j]), b[j], acc);
    }
    return __fmul_rn(simple_wave_sum(acc), scale);
}

struct SimpleTrain {
    const float* ent; int64_t ld_ent; const float* rel; int64_t ld_rel; int32_t k_int; float scale;
    const int32_t* pos; int64_t B; int32_t eta; const int32_t* codes;
    float* scores_pos; float* scores_neg;               // forward
    const float* g_pos; const float* g_neg;             // backward: dL/dscore
    float* contrib_ent; float* contrib_rel; int64_t ldc;
};

__global__ __launch_bounds__(256) void score_simple_kernel(const float* __restrict__ ent, int64_t ld_ent, const float* __restrict__ rel,
                                                           int64_t ld_rel, int k_int, float scale, const int32_t* __restrict__ spo, int64_t n,
                                                           float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (t >= n) return;   // (no workgroup barrier below)
    const float f = simple_score(ent + (int64_t)spo[3 * t] * ld_ent, rel + (int64_t)spo[3 * t + 1] * ld_rel,
                                 ent + (int64_t)spo[3 * t + 2] * ld_ent, k_int >> 1, scale, lane);
    if (lane == 0) out[t] = f;
}

// scores of a positive and its eta negatives (eta-major codes: replacement | keep_subject << 31)
__global__ __launch_bounds__(256) void simple_forward_kernel(const SimpleTrain P) {
    const int lane = threadIdx.x & 63;
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (g >= P.B) return;   // (no workgroup barrier below)
    const int half = P.k_int >> 1;
    const float* es = P.ent + (int64_t)P.pos[3 * g] * P.ld_ent;
    const float* ep = P.rel + (int64_t)P.pos[3 * g + 1] * P.ld_rel;
    const float* eo = P.ent + (int64_t)P.pos[3 * g + 2] * P.ld_ent;
    const float f = simple_score(es, ep, eo, half, P.scale, lane);
    if (lane == 0) P.scores_pos[g] = f;
    for (int j = 0; j < P.eta; ++j) {
        const int32_t code = P.codes[(int64_t)j * P.B + g];
        const float* er = P.ent + (int64_t)(code & 0x7fffffff) * P.ld_ent;
        const float fn = code < 0 ? simple_score(es, ep, er, half, P.scale, lane) : simple_score(er, ep, eo, half, P.scale, lane);
        if (lane == 0) P.scores_neg[(int64_t)j * P.B + g] = fn;
    }
}

// gradient rows of a positive group in the contribution layout of every model (transe_p_backward_kernel): slot g = dE[s], B + g =
// dE[o], 2B + jB + g = the replacement of negative j, relation slot g = dR[p].  Every slot is written over its k_int columns; the
// shared rows accumulate in their slots, positive first, negatives in ascending j, by the lane that owns the column.  A triple
// with s == o (or a replacement equal to the kept entity) has its two entity rows in two slots of one destination: the apply adds them.
//   w = g * scale;  da = w (r o swap(b));  db = swap(w (r o a));  dr = w (a o swap(b))
__global__ __launch_bounds__(256) void simple_backward_kernel(const SimpleTrain P) {
    const int lane = threadIdx.x & 63;
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (g >= P.B) return;   // (no workgroup barrier below)
    const int half = P.k_int >> 1;
    const float* es = P.ent + (int64_t)P.pos[3 * g] * P.ld_ent;
    const float* ep = P.rel + (int64_t)P.pos[3 * g + 1] * P.ld_rel;
    const float* eo = P.ent + (int64_t)P.pos[3 * g + 2] * P.ld_ent;
    float* cs = P.contrib_ent + g * P.ldc;
    float* co = P.contrib_ent + (P.B + g) * P.ldc;
    float* cp = P.contrib_rel + g * P.ldc;
    {
        const float w = __fmul_rn(P.g_pos[g], P.scale);
        for (int c = lane; c < half; c += 64) {
            const float a_l = es[c], a_h = es[half + c], r_l = ep[c], r_h = ep[half + c], b_l = eo[c], b_h = eo[half + c];
            cs[c] = __fmul_rn(w, __fmul_rn(r_l, b_h)); cs[half + c] = __fmul_rn(w, __fmul_rn(r_h, b_l));
            co[half + c] = __fmul_rn(w, __fmul_rn(r_l, a_l)); co[c] = __fmul_rn(w, __fmul_rn(r_h, a_h));
            cp[c] = __fmul_rn(w, __fmul_rn(a_l, b_h)); cp[half + c] = __fmul_rn(w, __fmul_rn(a_h, b_l));
        }
    }
    for (int j = 0; j < P.eta; ++j) {
        const int32_t code = P.codes[(int64_t)j * P.B + g];
        const bool keep_s = code < 0;   // subject kept: the OBJECT was replaced
        const float* er = P.ent + (int64_t)(code & 0x7fffffff) * P.ld_ent;
        const float* a = keep_s ? es : er;
        const float* b = keep_s ? er : eo;
        float* cr = P.contrib_ent + (2 * P.B + (int64_t)j * P.B + g) * P.ldc;
        const float w = __fmul_rn(P.g_neg[(int64_t)j * P.B + g], P.scale);
        for (int c = lane; c < half; c += 64) {
            const float a_l = a[c], a_h = a[half + c], r_l = ep[c], r_h = ep[half + c], b_l = b[c], b_h = b[half + c];
            const float da_l = __fmul_rn(w, __fmul_rn(r_l, b_h)), da_h = __fmul_rn(w, __fmul_rn(r_h, b_l));
            const float db_h = __fmul_rn(w, __fmul_rn(r_l, a_l)), db_l = __fmul_rn(w, __fmul_rn(r_h, a_h));
            cp[c] = __fadd_rn(cp[c], __fmul_rn(w, __fmul_rn(a_l, b_h)));
            cp[half + c] = __fadd_rn(cp[half + c], __fmul_rn(w, __fmul_rn(a_h, b_l)));
            if (keep_s) {
                cs[c] = __fadd_rn(cs[c], da_l); cs[half + c] = __fadd_rn(cs[half + c], da_h);
                cr[c] = db_l; cr[half + c] = db_h;
            } else {
                co[c] = __fadd_rn(co[c], db_l); co[half + c] = __fadd_rn(co[half + c], db_h);
                cr[c] = da_l; cr[half + c] = da_h;
            }
        }
    }
}

}  // namespace

int simple_check(int32_t k_int, int64_t ld_ent, int64_t ld_rel) {
    EMG_REQUIRE(k_int > 0 && k_int % 2 == 0 && ld_ent >= k_int && ld_rel >= k_int,
                "EMG_SIMPLE: k_int = %d must be even (entity rows [h | t], relation rows [r | r_inv]) and no wider than the row strides", (int)k_int);
    return EMG_OK;
}

int simple_forward(const float* ent, int64_t ld_ent, const float* rel, int64_t ld_rel, int32_t k_int, float scale, const int32_t* pos,
                   int64_t B, int32_t eta, const int32_t* codes, int32_t flags, float* scores_pos, float* scores_neg, void* stream) {
    int rc = simple_check(k_int, ld_ent, ld_rel);
    if (rc != EMG_OK) return rc;
    EMG_REQUIRE(flags == EMG_SCORE_FINAL, "EMG_SIMPLE: no partial (column-slab) scores");
    EMG_REQUIRE(B >= 0 && eta >= 0 && cdiv(B * 64, 256) < ((int64_t)1 << 31), "EMG_SIMPLE: bad sizes");
    if (B == 0) return EMG_OK;
    if (eta == 0) {
        hipLaunchKernelGGL(score_simple_kernel, dim3((unsigned)cdiv(B * 64, 256)), dim3(256), 0, (hipStream_t)stream, ent, ld_ent, rel, ld_rel,
                           (int)k_int, scale, pos, B, scores_pos);
    } else {
        EMG_REQUIRE(codes && scores_neg, "emg_train_forward: eta>0 needs codes and scores_neg");
        SimpleTrain T{};
        T.ent = ent; T.ld_ent = ld_ent; T.rel = rel; T.ld_rel = ld_rel; T.k_int = k_int; T.scale = scale; T.pos = pos; T.B = B; T.eta = eta;
        T.codes = codes; T.scores_pos = scores_pos; T.scores_neg = scores_neg;
        hipLaunchKernelGGL(simple_forward_kernel, dim3((unsigned)cdiv(B * 64, 256)), dim3(256), 0, (hipStream_t)stream, T);
    }
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

// the caller (emg_score.hip: backward_step) has checked the pointers, ldc >= k_int, the external dL/dscore and simple_check
int simple_backward(const emg_backward_args* a, void* stream) {
    EMG_REQUIRE(cdiv(a->B * 64, 256) < ((int64_t)1 << 31), "EMG_SIMPLE: batch too large");
    SimpleTrain T{};
    T.ent = a->ent; T.ld_ent = a->ld_ent; T.rel = a->rel; T.ld_rel = a->ld_rel; T.k_int = a->k_int; T.scale = a->scale; T.pos = a->pos;
    T.B = a->B; T.eta = a->eta; T.codes = a->codes; T.g_pos = a->g_pos; T.g_neg = a->g_neg;
    T.contrib_ent = a->contrib_ent; T.contrib_rel = a->contrib_rel; T.ldc = a->ldc;
    hipLaunchKernelGGL(simple_backward_kernel, dim3((unsigned)cdiv(a->B * 64, 256)), dim3(256), 0, (hipStream_t)stream, T);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

}  // namespace emg
