// emg_rank_typed.hip — TYPED ranking: every query row is counted against the candidate pool of ITS group (the domain or range of
// its relation: the local closed-world assumption of Krompass et al. 2015; LibKGE's type-constrained ranking), all groups in ONE
// launch.  Contract: include/emgraph_hip.h, emg_eval_count_grouped; the host side: evaluation/ranking.py, _rank_typed.
//
// The score of a (row, candidate) pair is the canonical chain of emg_chain.hpp — chain_score's steps, k ascending, one accumulator
// register per pair — so the counters equal what emg_eval_count(..., cand = the pool) returns for the row: the typed rank of a
// triple is the rank the entities_subset path gives it, bit for bit.
//
// SCHEDULE (no workspace, no scheduling launch, no host read).  The rows are cut into fixed windows of 64 consecutive rows.  A
// window holds one or more SEGMENTS: maximal runs of rows with the same group id.  Workgroup (window w, split c) walks the
// segments of w and, for each, the candidate tiles c, c + csplit, c + 2 csplit, ... of that group's pool: a tile is the rows of
// ONE segment (at most 64) against at most 64 pool members, gathered by id into LDS.  Work is sum_g rows_g |pool_g| rounded up
// to tiles; a group with no rows is never met, a row with a negative group forms segments that are skipped, a pool smaller than
// a tile is one masked tile, a group whose rows straddle two windows is two segments.  The order of the groups is free (the
// kernel only looks at runs); rows sorted by group give the fewest segments.
#include "emg_chain.hpp"   // chain_score's steps (rotate_step, chain_step)

// The canonical order is only canonical if the compiler never fuses a*b+c on its own: every fused multiply-add in this file is
// an explicit __fmaf_rn.
#pragma clang fp contract(off)

namespace emg {

__device__ __forceinline__ int typed_cmp_int(float score) { return (int)__fmul_rn(score, 100000.0f); }   // as emg_rank.hip (EmbeddingModel.py:2010-2014)

struct GroupedParams {
    const float* Q; int64_t ldq; const int32_t* pos_int; int64_t n_rows; const int32_t* row_group;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const int64_t* pool_ptr; const int32_t* pool_idx; int64_t n_groups;
    int32_t k_int; float scale; int32_t model; int32_t csplit;
    int32_t* cnt_gt; int32_t* cnt_eq;
};

// 64 rows x 64 candidates per tile, 4 x 4 per thread; a k-tile is 32 LDS rows: 32 coordinates, or RotatE's 16 real parts above
// its 16 imaginary parts (count_transe_kernel's and count_rotate_kernel's tiles, emg_rank.hip)
constexpr int GQ = 64, GE = 64, GK = 32, GJ = 16;

// KIND: 0 fmaf(q, e, acc) (DistMult, ComplEx, HolE); 1 acc + |q - e| (TransE-L1); 2 fmaf(d, d, acc) (TransE-L2);
//       3 acc + |q - e|^ord, ord = inf: max (TransE-p); 4 RotatE
template <int KIND>
__global__ __launch_bounds__(256) void count_grouped_kernel(const GroupedParams P) {
    __shared__ __attribute__((aligned(16))) float Qs[GK * GQ];
    __shared__ __attribute__((aligned(16))) float Es[GK * GE];
    __shared__ int pos_s[GQ];
    __shared__ int grp_s[GQ];
    __shared__ unsigned gt_s[GQ];
    __shared__ unsigned eq_s[GQ];

    const int64_t win = (int64_t)blockIdx.x / P.csplit;
    const int c = (int)((int64_t)blockIdx.x % P.csplit);
    const int64_t row0 = win * GQ;
    const int tid = threadIdx.x;
    const int tq = tid & 15, te = tid >> 4;
    const int lrow = tid & 63, lkq = tid >> 6;   // loader: row lrow, LDS rows 4 lkq .. 4 lkq + 3 of each half of the k-tile
    const int half = P.k_int >> 1;               // (RotatE)
    const int n_steps = KIND == 4 ? half : P.k_int, step_tile = KIND == 4 ? GJ : GK;
    const bool p_inf = KIND == 3 && isinf(P.scale);

    if (tid < GQ) {
        const int64_t qr = row0 + tid;
        const bool ok = qr < P.n_rows;
        const int g = ok ? P.row_group[qr] : -1;
        grp_s[tid] = (g >= 0 && (int64_t)g < P.n_groups) ? g : -1;
        pos_s[tid] = ok ? P.pos_int[qr] : 0x7fffffff;
        gt_s[tid] = 0u;
        eq_s[tid] = 0u;
    }
    __syncthreads();

    unsigned cgt[4] = {0u, 0u, 0u, 0u}, ceq[4] = {0u, 0u, 0u, 0u};
    for (int a0 = 0; a0 < GQ;) {   // the segments of the window: block-uniform
        const int g = grp_s[a0];
        int a1 = a0 + 1;
        while (a1 < GQ && grp_s[a1] == g) ++a1;
        if (g >= 0) {
            const int64_t p0 = P.pool_ptr[g];
            const int64_t len = P.pool_ptr[g + 1] - p0;
            const int64_t n_ct = (len > 0 && p0 >= 0) ? (len + GE - 1) / GE : 0;
            const bool qok = lrow >= a0 && lrow < a1;
            const float* qptr = P.Q + (row0 + (qok ? lrow : a0)) * P.ldq;
            for (int64_t ct = c; ct < n_ct; ct += P.csplit) {
                const int64_t cbase = p0 + ct * GE;
                const int ncand = (int)min((int64_t)GE, len - ct * GE);
                bool eok = lrow < ncand;
                const int32_t eid = eok ? P.pool_idx[cbase + lrow] : 0;
                eok = eok && eid >= 0 && (int64_t)eid < P.n_ent;   // (an id outside the table is never read, and never counted)
                const float* eptr = P.ent + (eok ? (int64_t)eid : 0) * P.ld_ent;
                float acc[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
                for (int s0 = 0; s0 < n_steps; s0 += step_tile) {
                    float qv[2][4], ev[2][4];
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            // column of LDS row kl(h, cc): coordinate s0 + kl, or RotatE's re (h = 0) / im (h = 1) of coordinate s0 + 4 lkq + cc
                            const int st = KIND == 4 ? s0 + 4 * lkq + cc : s0 + 4 * (lkq + 4 * h) + cc;
                            const int col = KIND == 4 ? h * half + st : st;
                            const bool in = st < n_steps;
                            qv[h][cc] = (qok && in) ? qptr[col] : 0.f;
                            ev[h][cc] = (eok && in) ? eptr[col] : 0.f;
                        }
                    __syncthreads();
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            const int kl = KIND == 4 ? h * GJ + 4 * lkq + cc : 4 * (lkq + 4 * h) + cc;
                            Qs[kl * GQ + lrow] = qv[h][cc];
                            Es[kl * GE + lrow] = ev[h][cc];
                        }
                    __syncthreads();
                    const int sn = min(step_tile, n_steps - s0);   // exactly chain_score's steps: a tail tile takes no extra one
                    if constexpr (KIND == 4) {
                        for (int j = 0; j < sn; ++j) {
                            const float4 qr4 = *reinterpret_cast<const float4*>(&Qs[j * GQ + 4 * tq]);
                            const float4 qi4 = *reinterpret_cast<const float4*>(&Qs[(GJ + j) * GQ + 4 * tq]);
                            const float4 er4 = *reinterpret_cast<const float4*>(&Es[j * GE + 4 * te]);
                            const float4 ei4 = *reinterpret_cast<const float4*>(&Es[(GJ + j) * GE + 4 * te]);
                            const float qr[4] = {qr4.x, qr4.y, qr4.z, qr4.w}, qi[4] = {qi4.x, qi4.y, qi4.z, qi4.w};
                            const float er[4] = {er4.x, er4.y, er4.z, er4.w}, ei[4] = {ei4.x, ei4.y, ei4.z, ei4.w};
#pragma unroll
                            for (int a = 0; a < 4; ++a) {
#pragma unroll
                                for (int b = 0; b < 4; ++b) acc[a][b] = rotate_step(qr[a], qi[a], er[b], ei[b], acc[a][b]);
                                // four square roots in flight, not sixteen: each keeps two lane masks in scalar registers, and
                                // sixteen at once spill 30 of them (the compile's report); the arithmetic is the same
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    } else {
#pragma unroll 4
                        for (int k = 0; k < sn; ++k) {
                            const float4 q4 = *reinterpret_cast<const float4*>(&Qs[k * GQ + 4 * tq]);
                            const float4 e4 = *reinterpret_cast<const float4*>(&Es[k * GE + 4 * te]);
                            const float q[4] = {q4.x, q4.y, q4.z, q4.w};
                            const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                            for (int a = 0; a < 4; ++a)
#pragma unroll
                                for (int b = 0; b < 4; ++b) {
                                    if constexpr (KIND == 3) {
                                        const float d = fabsf(__fsub_rn(q[a], e[b]));
                                        acc[a][b] = p_inf ? fmaxf(acc[a][b], d) : __fadd_rn(acc[a][b], powf(d, P.scale));
                                    } else {
                                        acc[a][b] = chain_step<KIND>(q[a], e[b], acc[a][b]);
                                    }
                                }
                        }
                    }
                }
                // ---- the model's final step, the comparison, the counts (rows of this segment x members of this tile) ----
                bool cok[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = 4 * te + b;
                    const int32_t id = col < ncand ? P.pool_idx[cbase + col] : -1;
                    cok[b] = id >= 0 && (int64_t)id < P.n_ent;
                }
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int ql = 4 * tq + a;
                    const bool rok = ql >= a0 && ql < a1;
                    const int p = pos_s[ql];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        float v;
                        if constexpr (KIND == 0) v = P.model == EMG_HOLE ? __fmul_rn(acc[a][b], P.scale) : acc[a][b];
                        else if constexpr (KIND == 2) v = -sqrtf(acc[a][b]);
                        else if constexpr (KIND == 3) v = p_inf ? -acc[a][b] : -powf(acc[a][b], 1.0f / P.scale);
                        else v = -acc[a][b];
                        const int ci = typed_cmp_int(v);
                        const bool on = rok && cok[b];
                        cgt[a] += (unsigned)(on && ci > p);
                        ceq[a] += (unsigned)(on && ci == p);
                    }
                }
            }
        }
        a0 = a1;
    }
    // 16 threads share a query row; ONE atomic per row, counter and workgroup reaches memory
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (cgt[a]) atomicAdd(&gt_s[4 * tq + a], cgt[a]);
        if (ceq[a]) atomicAdd(&eq_s[4 * tq + a], ceq[a]);
    }
    __syncthreads();
    if (tid < GQ) {
        const int64_t qr = row0 + tid;
        if (qr < P.n_rows) {
            if (gt_s[tid]) atomicAdd(&P.cnt_gt[qr], (int)gt_s[tid]);
            if (eq_s[tid]) atomicAdd(&P.cnt_eq[qr], (int)eq_s[tid]);
        }
    }
}

typedef void (*GroupedKernel)(const GroupedParams);
static GroupedKernel grouped_form(int model) {
    switch (model) {
        case EMG_TRANSE_L1: return count_grouped_kernel<1>;
        case EMG_TRANSE_L2: return count_grouped_kernel<2>;
        case EMG_TRANSE_P: return count_grouped_kernel<3>;
        case EMG_ROTATE: return count_grouped_kernel<4>;
        default: return count_grouped_kernel<0>;
    }
}

// workgroups per window: enough of them to fill the device when the windows are few, never more than a pool can have tiles
constexpr int64_t kGroupedBlocks = 4096, kGroupedSplitMax = 256;

}  // namespace emg

using namespace emg;

extern "C" int emg_eval_count_grouped(int model, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                                      const int32_t* row_group, const float* ent, int64_t n_ent, int64_t ld_ent,
                                      const int64_t* pool_ptr, const int32_t* pool_idx, int64_t n_groups, int32_t k_int, float scale,
                                      int32_t* cnt_gt, int32_t* cnt_eq, void* stream) {
    model = chain_model(model);
    EMG_REQUIRE(model >= 0 && model <= EMG_ROTATE, "emg_eval_count_grouped: unknown model id %d", model);
    EMG_REQUIRE(n_rows >= 0 && n_ent >= 0 && n_groups >= 0 && k_int > 0 && ldq >= k_int && ld_ent >= k_int, "emg_eval_count_grouped: bad sizes");
    EMG_REQUIRE(n_ent < ((int64_t)1 << 31) && n_groups < ((int64_t)1 << 31), "emg_eval_count_grouped: ids must fit 31 bits");
    EMG_REQUIRE(model != EMG_ROTATE || k_int % 2 == 0, "emg_eval_count_grouped: EMG_ROTATE: odd k_int %d", k_int);
    EMG_REQUIRE(model != EMG_TRANSE_P || scale > 0.f, "emg_eval_count_grouped: EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive");
    if (n_rows == 0 || n_groups == 0 || n_ent == 0) return EMG_OK;
    EMG_REQUIRE(Q && pos_int && row_group && ent && pool_ptr && cnt_gt && cnt_eq, "emg_eval_count_grouped: null pointer");
    GroupedParams P{};
    P.Q = Q; P.ldq = ldq; P.pos_int = pos_int; P.n_rows = n_rows; P.row_group = row_group; P.ent = ent; P.n_ent = n_ent; P.ld_ent = ld_ent;
    P.pool_ptr = pool_ptr; P.pool_idx = pool_idx; P.n_groups = n_groups; P.k_int = k_int; P.scale = scale; P.model = model;
    P.cnt_gt = cnt_gt; P.cnt_eq = cnt_eq;
    const int64_t windows = cdiv(n_rows, GQ);
    int64_t csplit = cdiv(kGroupedBlocks, windows);
    if (csplit > kGroupedSplitMax) csplit = kGroupedSplitMax;
    if (csplit > cdiv(n_ent, GE)) csplit = cdiv(n_ent, GE);
    P.csplit = (int32_t)csplit;
    EMG_REQUIRE(windows * csplit < ((int64_t)1 << 31), "emg_eval_count_grouped: grid too large");
    hipLaunchKernelGGL(grouped_form(model), dim3((unsigned)(windows * csplit)), dim3(256), 0, (hipStream_t)stream, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
