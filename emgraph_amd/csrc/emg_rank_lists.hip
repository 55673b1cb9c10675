// emg_rank_lists.hip — SAMPLED ranking: every query row is counted against a candidate list of ITS OWN (OGB's head_neg / tail_neg
// arrays, DGL-KE's neg_sample_size_eval, PyKEEN's SampledRankBasedEvaluator), with the row's known positives excluded in the
// same launch, and the device draw of such lists.  Contract: include/emgraph_hip.h, emg_eval_count_lists and
// emg_eval_draw_candidates; the host side: evaluation/ranking.py, _rank_lists.
//
// The score of a (row, candidate) pair is the canonical chain of emg_chain.hpp — chain_score's steps, k ascending, one accumulator
// register per pair — so a pair has the bits emg_eval_scores_dense writes for it, and the counters equal what
// emg_eval_filter_count adds for the same list.
//
// WHAT WAS CHOSEN, AND WHY
//   Schedule.  A wave owns ONE query row and takes its list 64 candidates at a time, one lane per candidate.  A list is split
//     over `nsplit` waves (batch b goes to wave b mod nsplit) only when the rows alone do not fill the device: nsplit =
//     ceil(kListWaves / n_rows), at most the number of batches.  At 16384 rows every wave walks its whole list.
//   Query row.  One coalesced load per slice and wave — lane l holds the query's value for chain step l of the slice — issued with
//     the candidate slice it belongs to, and broadcast to the chain by v_readlane (a scalar operand of the step): no LDS traffic
//     for it.  Left as plain reads of the wave-uniform address, the compiler made each a vector load with a full vmcnt(0) wait in
//     the chain, which also drained the slice in flight.
//   Candidate rows (16-byte aligned rows: VEC).  A slice of LK = 32 coordinates of the 64 candidate rows is gathered with
//     coalesced loads — 8 lanes x 16 B = one 128-byte line per row and instruction, 8 rows per instruction, 8 instructions per
//     slice — into the wave's own LDS region (row stride 36 floats: the ds_write_b128 of 8 lanes fills one row's 32 consecutive
//     banks, the ds_read_b128 of lane l starts at bank 36 l mod 64 — 16 lanes of a read group, 16 different quads).  The next
//     slice is in flight under the current slice's chain.  RotatE's slice is 16 complex coordinates, [re 0..15 | im 0..15].
//   No load sits under a lane predicate (a predicated load is a branch, and hipcc drains every outstanding load at its join): a
//     lane without a candidate — padding, an excluded id, the list's end — borrows the id of the wave's first live lane, and a
//     16-byte piece past the row's end re-reads the row's last whole piece (the same line); neither value reaches a chain step of
//     a counted pair.  So an id outside [0, n_ent) is never used as an index.  A batch without a live lane is skipped.
//   What bounds it.  The kernel is gather-bound: 4 k_int bytes per pair from a table far larger than any cache (1600 B at ComplEx
//     k = 200), against ~200 chain steps.  Bytes in flight per CU are what hide an HBM miss (MI355X: 72 KiB per CU hide most of
//     it): a slice is 8 KiB per wave in registers on its way to LDS, the LDS region 9 KiB per wave, 36 KiB per workgroup of four
//     waves — four workgroups, 16 waves, 128 KiB of row bytes in flight per CU.  LK = 16 (rescore_pairs_kernel's slice) halves
//     that and asks for every 128-byte line twice.
//   Rows that are not 16-byte aligned (ld_ent % 4 != 0, or a misaligned base): every lane runs the chain over its candidate's row
//     straight from memory (the filter-count access pattern); k_int % 4 (RotatE: the half % 4) leftover coordinates of aligned
//     rows are read the same way after the staged slices.  RotatE rows are staged when k_int % 8 == 0 (both halves aligned).
//   Counters.  ballot + popcount per batch (wave-uniform scalars), ONE atomic per wave and field at the end.
//   No workspace, no host read, no second launch.
#include "emg_chain.hpp"   // chain_score's steps (rotate_step, chain_step)

// The canonical order is only canonical if the compiler never fuses a*b+c on its own: every fused multiply-add in this file is
// an explicit __fmaf_rn.
#pragma clang fp contract(off)

namespace emg {

__device__ __forceinline__ int lists_cmp_int(float score) { return (int)__fmul_rn(score, 100000.0f); }   // as emg_rank.hip (EmbeddingModel.py:2010-2014)

struct ListsParams {
    const float* Q; int64_t ldq; const int32_t* pos_int; int64_t n_rows;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const int32_t* cand; int64_t ld_cand; int32_t n_cand;
    const int64_t* excl_ptr; const int32_t* excl_idx;
    int32_t k_int; float scale; int32_t model; int32_t nsplit;
    int32_t* cnt_gt; int32_t* cnt_eq;
};

constexpr int LK = 32, LLD = LK + 4;     // coordinates of a staged slice; LDS row stride (floats)
constexpr int LW = 4;                    // waves per workgroup
constexpr int64_t kListWaves = 8192;     // waves wanted in the grid before lists are split: two rounds of 256 CUs x 16 waves

__device__ __forceinline__ void lists_lds_sync() {   // this wave's LDS writes are visible to its own later reads (emg_rank.hip: wave_lds_sync)
    __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// KIND: 0 fmaf(q, e, acc) (DistMult, ComplEx, HolE); 1 acc + |q - e| (TransE-L1); 2 fmaf(d, d, acc) (TransE-L2);
//       3 acc + |q - e|^ord, ord = inf: max (TransE-p); 4 RotatE
template <int KIND>
__device__ __forceinline__ float lists_step(float q, float e, float acc, bool p_inf, float ord) {
    if constexpr (KIND == 3) {
        const float d = fabsf(__fsub_rn(q, e));
        return p_inf ? fmaxf(acc, d) : __fadd_rn(acc, powf(d, ord));
    } else {
        return chain_step<KIND>(q, e, acc);
    }
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(64 * LW) void count_lists_kernel(const ListsParams P) {
    __shared__ __attribute__((aligned(16))) float es[VEC ? LW : 1][VEC ? 64 * LLD : 4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t w = (int64_t)blockIdx.x * LW + wave;   // wave-uniform
    const int64_t r = w / P.nsplit;
    const int split = (int)(w % P.nsplit);
    if (r >= P.n_rows) return;
    const float* __restrict__ q = P.Q + r * P.ldq;
    const int32_t* __restrict__ list = P.cand + r * P.ld_cand;
    const int p = P.pos_int[r];
    const bool p_inf = KIND == 3 && isinf(P.scale);
    const int half = P.k_int >> 1;   // (RotatE)
    int64_t x0 = 0, x1 = 0;          // the row's exclusion range
    if (P.excl_ptr) { x0 = P.excl_ptr[r]; x1 = P.excl_ptr[r + 1]; }
    // the staged part of the chain: steps [0, n_vec) (coordinates; RotatE: complex coordinates), whole 16-byte pieces only
    const int n_steps = KIND == 4 ? half : P.k_int;
    const int n_vec = VEC ? (n_steps & ~3) : 0;
    constexpr int LS = KIND == 4 ? LK / 2 : LK;   // chain steps per slice
    float* mye = es[VEC ? wave : 0];
    const int sub = lane >> 3, part = lane & 7;   // loader role: candidate (8 it + sub) of the wave's 64, 16-byte piece `part` of its slice
    // the piece's first coordinate inside a slice, and where the piece lies in the row: RotatE's pieces 4..7 are imaginary parts
    const int pstep = KIND == 4 ? 4 * (part & 3) : 4 * part;
    const int pbase = KIND == 4 ? (part >> 2) * half : 0;

    int gt = 0, eq = 0;   // wave-uniform
    for (int64_t c0 = 64 * (int64_t)split; c0 < P.n_cand; c0 += 64 * (int64_t)P.nsplit) {
        const int64_t ci = c0 + lane;
        int32_t id = ci < P.n_cand ? list[ci] : -1;
        bool live = id >= 0 && (int64_t)id < P.n_ent;
        if (live && x1 > x0) {   // is the id in the row's ascending exclusion list?
            int64_t a = x0, b = x1;   // the first entry >= id lies in [a, b]
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                if (P.excl_idx[mid] < id) a = mid + 1; else b = mid;
            }
            live = !(a < x1 && P.excl_idx[a] == id);
        }
        const unsigned long long lm = __ballot(live ? 1 : 0);
        if (lm == 0ull) continue;   // (wave-uniform)
        // a lane without a candidate reads the row of the first live lane: a row this wave is reading anyway
        const int32_t id_first = __builtin_amdgcn_readlane(id, __ffsll((long long)lm) - 1);
        const int32_t id_safe = live ? id : id_first;
        const float* __restrict__ er = P.ent + (int64_t)id_safe * P.ld_ent;
        float acc = 0.f;
        if constexpr (VEC) {
            if (n_vec > 0) {
                // (eight named registers, not an array: the array form of this loop was left in scratch memory by the compiler)
#define LISTS_X8(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define LISTS_PTR(i) const float* ep##i = P.ent + (int64_t)__shfl(id_safe, 8 * i + sub, 64) * P.ld_ent + pbase;
#define LISTS_DECL(i) float4 ev##i;
#define LISTS_LOAD(i) ev##i = *reinterpret_cast<const float4*>(ep##i + st);
#define LISTS_STAGE(i) *reinterpret_cast<float4*>(mye + (8 * i + sub) * LLD + 4 * part) = ev##i;
                LISTS_X8(LISTS_PTR)
                LISTS_X8(LISTS_DECL)
                // the query slice rides along: lane l holds the query's value for chain step l of the slice (RotatE: lanes 0..15 the
                // real parts, 16..31 the imaginary parts), broadcast to the chain with v_readlane
                const int ql = lane & (LS - 1);
                const float* qp = q + ((KIND == 4 && (lane & 16)) ? half : 0);
                float qv;
                int st = min(pstep, n_vec - 4);   // a piece past the staged part re-reads the row's last whole piece: never consumed
                LISTS_X8(LISTS_LOAD)
                qv = qp[min(ql, n_vec - 1)];
                for (int s0 = 0; s0 < n_vec; s0 += LS) {
                    lists_lds_sync();   // the previous slice has been consumed by every lane
                    LISTS_X8(LISTS_STAGE)
                    const float qc = qv;
                    lists_lds_sync();
                    if (s0 + LS < n_vec) {   // the next slice flies while this one is multiplied (wave-uniform)
                        st = min(s0 + LS + pstep, n_vec - 4);
                        LISTS_X8(LISTS_LOAD)
                        qv = qp[min(s0 + LS + ql, n_vec - 1)];
                    }
                    const int sn = min(LS, n_vec - s0);
                    auto qb = [&](int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qc), l)); };
#pragma unroll
                    for (int c = 0; c < LS / 4; ++c) {
                        if (4 * c < sn) {   // (wave-uniform)
                            if constexpr (KIND == 4) {
                                const float4 br = *reinterpret_cast<const float4*>(mye + lane * LLD + 4 * c);
                                const float4 bi = *reinterpret_cast<const float4*>(mye + lane * LLD + LK / 2 + 4 * c);
                                acc = rotate_step(qb(4 * c), qb(16 + 4 * c), br.x, bi.x, acc);
                                acc = rotate_step(qb(4 * c + 1), qb(16 + 4 * c + 1), br.y, bi.y, acc);
                                acc = rotate_step(qb(4 * c + 2), qb(16 + 4 * c + 2), br.z, bi.z, acc);
                                acc = rotate_step(qb(4 * c + 3), qb(16 + 4 * c + 3), br.w, bi.w, acc);
                            } else {
                                const float4 b = *reinterpret_cast<const float4*>(mye + lane * LLD + 4 * c);
                                acc = lists_step<KIND>(qb(4 * c), b.x, acc, p_inf, P.scale);
                                acc = lists_step<KIND>(qb(4 * c + 1), b.y, acc, p_inf, P.scale);
                                acc = lists_step<KIND>(qb(4 * c + 2), b.z, acc, p_inf, P.scale);
                                acc = lists_step<KIND>(qb(4 * c + 3), b.w, acc, p_inf, P.scale);
                            }
                        }
                    }
                }
#undef LISTS_X8
#undef LISTS_PTR
#undef LISTS_DECL
#undef LISTS_LOAD
#undef LISTS_STAGE
            }
        }
        // what was not staged (every step of rows that are not 16-byte aligned): the lane's own row, straight from memory
        for (int s = n_vec; s < n_steps; ++s) {
            if constexpr (KIND == 4) acc = rotate_step(q[s], q[half + s], er[s], er[half + s], acc);
            else acc = lists_step<KIND>(q[s], er[s], acc, p_inf, P.scale);
        }
        float v;   // the model's final step (chain_score's)
        if constexpr (KIND == 0) v = P.model == EMG_HOLE ? __fmul_rn(acc, P.scale) : acc;
        else if constexpr (KIND == 2) v = -sqrtf(acc);
        else if constexpr (KIND == 3) v = p_inf ? -acc : -powf(acc, 1.0f / P.scale);
        else v = -acc;
        const int cv = lists_cmp_int(v);
        gt += __popcll(__ballot((live && cv > p) ? 1 : 0));
        eq += __popcll(__ballot((live && cv == p) ? 1 : 0));
    }
    if (lane == 0) {
        if (gt) atomicAdd(&P.cnt_gt[r], gt);
        if (eq) atomicAdd(&P.cnt_eq[r], eq);
    }
}

typedef void (*ListsKernel)(const ListsParams);
static ListsKernel lists_form(int model, bool vec) {
    switch (model) {
        case EMG_TRANSE_L1: return vec ? count_lists_kernel<1, true> : count_lists_kernel<1, false>;
        case EMG_TRANSE_L2: return vec ? count_lists_kernel<2, true> : count_lists_kernel<2, false>;
        case EMG_TRANSE_P: return vec ? count_lists_kernel<3, true> : count_lists_kernel<3, false>;
        case EMG_ROTATE: return vec ? count_lists_kernel<4, true> : count_lists_kernel<4, false>;
        default: return vec ? count_lists_kernel<0, true> : count_lists_kernel<0, false>;
    }
}

// one thread per list entry; row order of emg_eval_build_queries (object-side rows first for EMG_EVAL_SPO / EMG_EVAL_S_O)
__global__ __launch_bounds__(256) void draw_candidates_kernel(int64_t n_q, int64_t q_offset, int side_mode, int32_t n_cand, uint64_t n_ent,
                                                              uint64_t seed, int32_t* __restrict__ cand, int64_t ld_cand, int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t row = t / n_cand;
    const uint32_t j = (uint32_t)(t - row * n_cand);
    const bool second = row >= n_q;   // (two-sided modes only: the subject-side rows)
    const uint64_t g = (uint64_t)(q_offset + (second ? row - n_q : row));
    const uint32_t sd = side_mode == EMG_EVAL_S ? 0u : (side_mode == EMG_EVAL_O ? 1u : (second ? 0u : 1u));
    const Philox4 o = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), j, sd, (uint32_t)seed, (uint32_t)(seed >> 32));
    cand[row * ld_cand + j] = (int32_t)__umul64hi(((uint64_t)o.v[2] << 32) | (uint64_t)o.v[1], n_ent);   // corruption_draw's reduction
}

}  // namespace emg

using namespace emg;

extern "C" int emg_eval_count_lists(int model, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                                    const float* ent, int64_t n_ent, int64_t ld_ent,
                                    const int32_t* cand, int64_t ld_cand, int32_t n_cand,
                                    const int64_t* excl_ptr, const int32_t* excl_idx,
                                    int32_t k_int, float scale, int32_t* cnt_gt, int32_t* cnt_eq, void* stream) {
    model = chain_model(model);
    EMG_REQUIRE(model >= 0 && model <= EMG_ROTATE, "emg_eval_count_lists: unknown model id %d", model);
    EMG_REQUIRE(n_rows >= 0 && n_ent >= 0 && n_cand >= 0 && k_int > 0 && ldq >= k_int && ld_ent >= k_int && ld_cand >= n_cand,
                "emg_eval_count_lists: bad sizes");
    EMG_REQUIRE(n_ent < ((int64_t)1 << 31), "emg_eval_count_lists: entity ids must fit 31 bits");
    EMG_REQUIRE(model != EMG_ROTATE || k_int % 2 == 0, "emg_eval_count_lists: EMG_ROTATE: odd k_int %d", k_int);
    EMG_REQUIRE(model != EMG_TRANSE_P || scale > 0.f, "emg_eval_count_lists: EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive");
    EMG_REQUIRE((excl_ptr == nullptr) == (excl_idx == nullptr), "emg_eval_count_lists: excl_ptr and excl_idx come together");
    if (n_rows == 0 || n_cand == 0 || n_ent == 0) return EMG_OK;   // (no entity: every id is padding)
    EMG_REQUIRE(Q && pos_int && ent && cand && cnt_gt && cnt_eq, "emg_eval_count_lists: null pointer");
    ListsParams P{};
    P.Q = Q; P.ldq = ldq; P.pos_int = pos_int; P.n_rows = n_rows; P.ent = ent; P.n_ent = n_ent; P.ld_ent = ld_ent;
    P.cand = cand; P.ld_cand = ld_cand; P.n_cand = n_cand; P.excl_ptr = excl_ptr; P.excl_idx = excl_idx;
    P.k_int = k_int; P.scale = scale; P.model = model; P.cnt_gt = cnt_gt; P.cnt_eq = cnt_eq;
    const int64_t batches = cdiv(n_cand, 64);
    int64_t nsplit = cdiv(kListWaves, n_rows);
    if (nsplit > batches) nsplit = batches;
    P.nsplit = (int32_t)nsplit;
    const int64_t blocks = cdiv(n_rows * nsplit, LW);
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_eval_count_lists: grid too large");
    // staged gather: 16-byte aligned entity rows (RotatE: both halves of a row)
    const bool vec = aligned16(ent) && ld_ent % 4 == 0 && (model != EMG_ROTATE || k_int % 8 == 0);
    hipLaunchKernelGGL(lists_form(model, vec), dim3((unsigned)blocks), dim3(64 * LW), 0, (hipStream_t)stream, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_eval_draw_candidates(int64_t n_q, int64_t q_offset, int side_mode, int32_t n_cand, int64_t n_ent,
                                        uint64_t seed, int32_t* cand, int64_t ld_cand, void* stream) {
    EMG_REQUIRE(side_mode >= EMG_EVAL_S && side_mode <= EMG_EVAL_S_O, "emg_eval_draw_candidates: bad side_mode %d", side_mode);
    EMG_REQUIRE(n_q >= 0 && q_offset >= 0 && n_cand >= 0 && ld_cand >= n_cand, "emg_eval_draw_candidates: bad sizes");
    EMG_REQUIRE(n_ent >= 1 && n_ent < ((int64_t)1 << 31), "emg_eval_draw_candidates: n_ent must lie in [1, 2^31)");
    if (n_q == 0 || n_cand == 0) return EMG_OK;
    EMG_REQUIRE(cand, "emg_eval_draw_candidates: null pointer");
    const int64_t n_rows = side_mode >= EMG_EVAL_SPO ? 2 * n_q : n_q;
    const int64_t total = n_rows * n_cand, blocks = cdiv(total, 256);
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_eval_draw_candidates: grid too large");
    hipLaunchKernelGGL(draw_candidates_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_q, q_offset, side_mode, n_cand,
                       (uint64_t)n_ent, seed, cand, ld_cand, total);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
