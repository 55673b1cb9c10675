// emg_sampler.hpp — the SAMPLED corruption draw: Bernoulli side choice (Wang et al. 2014, TransH) and known-triple filtering with
// redraws, as ONE device routine for the three producers of corruption ids (emg_sampler.hip: corrupt_codes_sampled_kernel,
// emg_group_kernels.hpp: prepare_ids_body, emg_group_bucket.hip: slot_ids).  Contract: include/emgraph_hip.h, emg_sampler_bind.
// Not in the reference (protocol.py:598-641 draws a fair coin and a uniform replacement and never looks at the graph).
//
// Only the SAMPLED instantiations of the producers include a call of it: the forms that run with no sampler bound — and ride in
// front of the training step's big launches — contain none of this code.
#pragma once
#include "emg_common.hpp"

namespace emg {

constexpr int kCoarseMax = 1024;   // entries of the coarse index a workgroup stages in LDS (8 KB)

// the bound sampler as the kernels see it (emg_sampler validated and reduced: emg_sampler.hip)
struct SamplerDev {
    const uint32_t* keep_thr;        // [n_rel]; nullptr: the fair coin of corruption_draw
    const uint64_t* known;           // [n_known] ascending distinct keys (s * n_rel + p) * n_ent + o; nullptr: no filter
    int64_t n_known;
    uint64_t n_ent, n_rel;
    unsigned long long* stats;       // [3] rows, redrawn, known_left ([4] with pools: + typed_rows); nullptr: not counted
    int32_t retries;                 // T: attempts 0..T
    int32_t shift, n_coarse;         // coarse index: known[i << shift], i < n_coarse <= kCoarseMax
    int32_t pad0;
    const int64_t* pool_ptr;         // [2 n_rel + 1] typed negatives: group 2 p + keep_subject; nullptr: no pools
    const int32_t* pool_idx;         // the pools' members (global entity ids)
};

// the binding of the moment (emg_sampler_bind); false: nothing bound
bool sampler_current(SamplerDev* out);

// Every 2^shift-th key into LDS, by the whole workgroup (a __syncthreads() follows at the caller).  The first log2(n_coarse) levels
// of every search of the workgroup then cost LDS reads instead of dependent trips to L2 / HBM; the staging loads themselves are
// independent of each other (all in flight at once) and hit the same n_coarse lines in every workgroup of the launch.
__device__ __forceinline__ void sampler_stage_coarse(const SamplerDev& S, uint64_t* coarse) {
    if (!S.known) return;
    for (int i = threadIdx.x; i < S.n_coarse; i += blockDim.x) coarse[i] = S.known[(int64_t)i << S.shift];
}

// key in known[]?  LDS levels first, then the run of < 2^shift keys behind the coarse entry
__device__ __forceinline__ bool sampler_known(const SamplerDev& S, const uint64_t* coarse, uint64_t key) {
    int lo = -1, hi = S.n_coarse;   // coarse[lo] <= key < coarse[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (coarse[mid] <= key) lo = mid; else hi = mid;
    }
    if (lo < 0) return false;
    if (coarse[lo] == key) return true;
    int64_t a = (int64_t)lo << S.shift, b = a + ((int64_t)1 << S.shift);   // known[a] < key; the key, if there, lies in (a, b)
    if (b > S.n_known) b = S.n_known;
    while (b - a > 1) {
        const int64_t mid = (a + b) >> 1;
        const uint64_t v = S.known[mid];
        if (v == key) return true;
        if (v < key) a = mid; else b = mid;
    }
    return false;
}

// attempt t of row j: index in [0, n_choices) (t = 0: corruption_draw's index); o0: the four words of attempt 0
__device__ __forceinline__ Philox4 sampler_words(uint64_t seed, uint64_t counter, uint64_t j, uint32_t t) {
    return philox4x32_10((uint32_t)j, (uint32_t)(j >> 32) | (t << 24), (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)seed,
                         (uint32_t)(seed >> 32));
}
__device__ __forceinline__ uint32_t sampler_index(const Philox4& o, uint64_t n_choices) {
    return (uint32_t)__umul64hi(((uint64_t)o.v[2] << 32) | (uint64_t)o.v[1], n_choices);
}

// The sampled draw of corruption row j (global draw index) of a positive (s, p, o) under `side`: *keep = keep_subject,
// *repl = the replacement entity (after the pool mapping `elist`, or from the relation's typed pool).  The side comes from attempt 0 (forced sides stay forced);
// with a filter the replacement is redrawn while the candidate is a known triple, T times at most.  May be called under any
// divergence: the attempt loop runs while ANY lane of the wave that is here still searches (a wave-uniform branch), and the
// three counts are ballots over those lanes, added by the first of them.
__device__ __forceinline__ void sampled_draw(const SamplerDev& S, const uint64_t* coarse, uint64_t seed, uint64_t counter, uint64_t j,
                                             uint64_t n_choices, const int32_t* __restrict__ elist, int side, int32_t s, int32_t p, int32_t o,
                                             uint32_t* keep_out, uint32_t* repl_out) {
    Philox4 w = sampler_words(seed, counter, j, 0u);
    uint32_t keep = w.v[0] & 1u;
    if (S.keep_thr && (uint64_t)(uint32_t)p < S.n_rel && p >= 0) keep = w.v[3] < S.keep_thr[p] ? 1u : 0u;
    if (side == EMG_SIDE_O) keep = 1u;       // protocol.py:606
    else if (side == EMG_SIDE_S) keep = 0u;  // :607-608
    // typed negatives: the replacement comes from the pool of the row's relation and side (group 2 p + keep: the subject kept means
    // the object is replaced, from the RANGE pool); an empty pool, or a relation out of range, draws as ever.  The same Philox
    // words: only the multiplier and the lookup change
    const int32_t* tpool = nullptr;
    uint64_t tlen = 0;
    if (S.pool_ptr && p >= 0 && (uint64_t)(uint32_t)p < S.n_rel) {
        const int64_t g = 2 * (int64_t)p + (int64_t)keep, a = S.pool_ptr[g], b = S.pool_ptr[g + 1];
        if (b > a) { tpool = S.pool_idx + a; tlen = (uint64_t)(b - a); }
    }
    uint32_t idx = sampler_index(w, tpool ? tlen : n_choices);
    uint32_t repl = (tpool ? (uint32_t)tpool[idx] : (elist ? (uint32_t)elist[idx] : idx)) & 0x7fffffffu;
    bool redrawn = false, left = false;
    if (S.known) {
        // the part of the key the attempts share: (s, p, .) or (., p, o)
        const uint64_t us = (uint64_t)(uint32_t)s, up = (uint64_t)(uint32_t)p, uo = (uint64_t)(uint32_t)o;
        const bool keyed = s >= 0 && p >= 0 && o >= 0 && us < S.n_ent && up < S.n_rel && uo < S.n_ent;   // (else: no triple of K)
        bool searching = true;
        for (uint32_t t = 0u;; ++t) {
            if (searching) {
                const uint64_t key = keep ? (us * S.n_rel + up) * S.n_ent + (uint64_t)repl : ((uint64_t)repl * S.n_rel + up) * S.n_ent + uo;
                const bool in = keyed && (uint64_t)repl < S.n_ent && sampler_known(S, coarse, key);
                if (!in || t == (uint32_t)S.retries) { searching = false; left = in; }
            }
            if (!__any(searching ? 1 : 0)) break;
            if (searching) {
                w = sampler_words(seed, counter, j, t + 1u);
                idx = sampler_index(w, tpool ? tlen : n_choices);
                repl = (tpool ? (uint32_t)tpool[idx] : (elist ? (uint32_t)elist[idx] : idx)) & 0x7fffffffu;
                redrawn = true;
            }
        }
    }
    if (S.stats) {
        const unsigned long long here = __ballot(1), m_re = __ballot(redrawn ? 1 : 0), m_left = __ballot(left ? 1 : 0);
        if ((int)__lane_id() == __ffsll((long long)here) - 1) {
            atomicAdd(S.stats + 0, (unsigned long long)__popcll(here));
            if (m_re) atomicAdd(S.stats + 1, (unsigned long long)__popcll(m_re));
            if (m_left) atomicAdd(S.stats + 2, (unsigned long long)__popcll(m_left));
        }
        if (S.pool_ptr) {   // (a fourth counter only where pools are bound: an old-size caller's stats stay [3])
            const unsigned long long m_typed = __ballot(tpool ? 1 : 0);
            if (m_typed && (int)__lane_id() == __ffsll((long long)here) - 1) atomicAdd(S.stats + 3, (unsigned long long)__popcll(m_typed));
        }
    }
    *keep_out = keep;
    *repl_out = repl;
}

}  // namespace emg
