// emg_chain.hpp — the canonical score chain of the 1-vs-all kernels (emg_rank.hip, emg_topn.hip).
//
// CANONICAL ORDER: every score is the chain acc_{k+1} = fmaf(q_k, e_k, acc_k), k ascending from acc_0 = +0
// (TransE-L1: acc + |q_k - e_k|; L2: fmaf(d,d,acc)), then the model's final step.  Every kernel that includes
// this header produces exactly that chain, so a (query row, entity) pair has the same bits wherever it is scored.
#pragma once
#include "emg_common.hpp"

// The canonical order is only canonical if the compiler never fuses a*b+c on its own: every fused multiply-add
// of the including file is an explicit __fmaf_rn / MFMA.
#pragma clang fp contract(off)

namespace emg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

typedef float float16v __attribute__((ext_vector_type(16)));

// RotatE's chain step on complex coordinate j (rows [re | im]): acc + |q_j - e_j|, the modulus unfused — subtract, two products,
// their sum, the square root, the add: each one correctly rounded operation, so a host restates the chain to the bit
__device__ __forceinline__ float rotate_step(float q_re, float q_im, float e_re, float e_im, float acc) {
    const float dr = __fsub_rn(q_re, e_re), di = __fsub_rn(q_im, e_im);
    return __fadd_rn(acc, sqrtf(__fadd_rn(__fmul_rn(dr, dr), __fmul_rn(di, di))));
}

// canonical chain of one (query row, entity row) pair
__device__ __forceinline__ float chain_score(int model, const float* __restrict__ q, const float* __restrict__ e, int k_int,
                                             float scale) {
    float acc = 0.f;
    if (model == EMG_ROTATE) {   // -sum_j |q_j - e_j| over the k_int / 2 complex coordinates
        const int n = k_int / 2;
        for (int j = 0; j < n; ++j) acc = rotate_step(q[j], q[n + j], e[j], e[n + j], acc);
        return -acc;
    }
    if (model == EMG_TRANSE_L1) {
        for (int k = 0; k < k_int; ++k) acc = __fadd_rn(acc, fabsf(__fsub_rn(q[k], e[k])));
        return -acc;
    }
    if (model == EMG_TRANSE_L2) {
        for (int k = 0; k < k_int; ++k) {
            const float d = __fsub_rn(q[k], e[k]);
            acc = __fmaf_rn(d, d, acc);
        }
        return -sqrtf(acc);
    }
    if (model == EMG_TRANSE_P) {   // any positive order (scale = ord): -(sum |d|^ord)^(1/ord); ord = inf: -max |d|
        if (isinf(scale)) {
            for (int k = 0; k < k_int; ++k) acc = fmaxf(acc, fabsf(__fsub_rn(q[k], e[k])));
            return -acc;
        }
        for (int k = 0; k < k_int; ++k) acc = __fadd_rn(acc, powf(fabsf(__fsub_rn(q[k], e[k])), scale));
        return -powf(acc, 1.0f / scale);
    }
    for (int k = 0; k < k_int; ++k) acc = __fmaf_rn(q[k], e[k], acc);
    return model == EMG_HOLE ? __fmul_rn(acc, scale) : acc;
}

__device__ __forceinline__ void load_frag4(float (&v)[4], const float* __restrict__ row, bool row_ok, int kbase, int k_int) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (row_ok && kbase + c < k_int) ? row[kbase + c] : 0.f;
}

// KIND: the chain step of chain_score — 0: fmaf(q, e, acc); 1: acc + |q - e|; 2: fmaf(d, d, acc), d = q - e
template <int KIND>
__device__ __forceinline__ float chain_step(float q, float e, float acc) {
    if constexpr (KIND == 0) return __fmaf_rn(q, e, acc);
    else if constexpr (KIND == 1) return __fadd_rn(acc, fabsf(__fsub_rn(q, e)));
    else { const float d = __fsub_rn(q, e); return __fmaf_rn(d, d, acc); }
}

}  // namespace emg
