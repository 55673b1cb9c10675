// emg_batchreg.hip — the batch-local Lp / N3 regulariser (DESIGN.md 0 A-29, 4.1 "Batch regulariser"; include/emgraph_hip.h has the
// contract).
//
// R = sum_i [ lambda_ent (N(E[s_i]) + N(E[o_i])) + lambda_rel N(R[p_i]) ] over the positives of a batch, every occurrence counted.
// Its gradient lives on 3 rows per positive: the kernel reads those rows and writes one gradient row each, with its destination,
// in the layout emg_relneg_backward uses — emg_group_dest / emg_apply_grouped sum a destination's rows.  Pure streaming, one launch:
//   a thread = (row slot, group of W columns); consecutive threads on consecutive columns of a row.  Row slots [0, B) are the
//   subject rows, [B, 2 B) the object rows, then — lambda_rel != 0 — B relation rows.  In the modulus form a thread takes columns
//   c .. c + W - 1 of BOTH halves (the pair (x_j, x_{j + k}) is its own): two loads, two stores, no LDS.
//   16-byte accesses (W = 4) where every row is 16-byte aligned and the column count of a pass (the half width in the modulus form)
//   is a multiple of 4; scalar ones (W = 1) otherwise.  The gradient rows are stored plainly: the grouping and the apply that
//   follow re-read them.
//   The value: a thread adds its f32 terms in double, ascending, scales by (double) coef_v; the workgroup adds its sum with ONE
//   atomic (block_add_double).  Same-address atomics retire one per ~10 ns, so the grid is a FEW LARGE workgroups
//   whose threads stride over the (row slot, column group) items: at most kBrMaxGroups atomics per launch — one workgroup of 256
//   threads per 256 items was 9600 atomics at bench.py's shape, 0.1 ms of a kernel whose bytes take 0.035.
// Every operation is one correctly rounded f32 operation, nothing contracted: tests/_batchreg_ref.py restates the rows to the bit.
// An id of `pos` outside its table is never followed (the thread takes row 0) and raises a device flag the entry point reads back.
#include <cmath>

#include "emg_chain.hpp"

// explicit operations only
#pragma clang fp contract(off)

namespace emg {
namespace {

constexpr int kBrThreads = 1024;     // 16 waves: block_add_double's limit
constexpr int kBrMaxGroups = 512;    // 8192 waves: the chip at 8 per SIMD

__device__ int32_t g_batchreg_bad;   // raised by a thread that met an id outside its table

struct BatchregParams {
    int32_t k_int;
    int32_t mod_ent, mod_rel;      // the table's rows are taken as pairs (x_j, x_{j + k_int / 2})
    float cg_ent, cv_ent, cg_rel, cv_rel;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const float* rel; int64_t n_rel; int64_t ld_rel;
    const int32_t* pos; int64_t B;
    float* contrib_ent; float* contrib_rel; int64_t ldc;
    int32_t* dest_ent; int32_t* dest_rel;
    double* value;
    int32_t nq_ent, nq_rel;        // column groups per row
    int64_t items_ent, items;      // threads with work: the entity rows' first
};

template <int W>
__device__ __forceinline__ void br_load(const float* __restrict__ row, int c, float (&v)[W]) {
    if constexpr (W == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(row + c);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = row[c];
    }
}

template <int W>
__device__ __forceinline__ void br_store(float* __restrict__ row, int c, const float (&v)[W]) {
    if constexpr (W == 4) {
        const f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(row + c) = t;
    } else {
        row[c] = v[0];
    }
}

// keeps a product out of a fused multiply-add: the `_rn` operations come from the device library with its own contraction flags,
// which the pragma above does not reach (emg_relneg.hip::rn_unfused has the case)
__device__ __forceinline__ float br_unfused(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// one coordinate of the plain form: its gradient entry and its f32 term of the value
template <int PW>
__device__ __forceinline__ float br_plain(float w, float cg, float* term) {
    const float aw = fabsf(w);
    if constexpr (PW == 1) {
        *term = aw;
        return __fmul_rn(cg, w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f));
    } else if constexpr (PW == 2) {
        *term = __fmul_rn(w, w);
        return __fmul_rn(cg, w);
    } else {
        *term = __fmul_rn(__fmul_rn(aw, aw), aw);
        return __fmul_rn(cg, __fmul_rn(aw, w));
    }
}

// one pair (a, b) = (x_j, x_{j + k}) of the modulus form: both gradient entries and the pair's f32 term of the value
template <int PW>
__device__ __forceinline__ void br_pair(float a, float b, float cg, float* ga, float* gb, float* term) {
    const float aa = br_unfused(__fmul_rn(a, a)), bb = br_unfused(__fmul_rn(b, b));
    const float s = __fadd_rn(aa, bb);
    if constexpr (PW == 2) {   // (the gradient is the plain form's)
        *term = s;
        *ga = __fmul_rn(cg, a);
        *gb = __fmul_rn(cg, b);
    } else {
        const float m = sqrtf(s);
        if constexpr (PW == 1) {
            *term = m;
            *ga = m != 0.f ? __fmul_rn(cg, __fdiv_rn(a, m)) : 0.f;
            *gb = m != 0.f ? __fmul_rn(cg, __fdiv_rn(b, m)) : 0.f;
        } else {
            *term = __fmul_rn(__fmul_rn(m, m), m);
            *ga = __fmul_rn(cg, __fmul_rn(m, a));
            *gb = __fmul_rn(cg, __fmul_rn(m, b));
        }
    }
}

template <int PW, int W>
__global__ __launch_bounds__(kBrThreads) void batchreg_kernel(const BatchregParams P) {
    double part = 0.0;   // (no early return: every thread reaches the workgroup's sum below)
    for (int64_t t = (int64_t)blockIdx.x * kBrThreads + threadIdx.x; t < P.items; t += (int64_t)gridDim.x * kBrThreads) {
        const bool is_rel = t >= P.items_ent;
        const int64_t u = is_rel ? t - P.items_ent : t;
        const int nq = is_rel ? P.nq_rel : P.nq_ent;
        const int64_t slot = u / nq;
        const int c = (int)(u - slot * nq) * W;
        const int64_t i = (is_rel || slot < P.B) ? slot : slot - P.B;
        const int col = is_rel ? 1 : (slot < P.B ? 0 : 2);
        int32_t id = P.pos[3 * i + col];
        if ((uint32_t)id >= (uint32_t)(is_rel ? P.n_rel : P.n_ent)) { g_batchreg_bad = 1; id = 0; }
        const float* row = is_rel ? P.rel + (int64_t)id * P.ld_rel : P.ent + (int64_t)id * P.ld_ent;
        float* out = (is_rel ? P.contrib_rel : P.contrib_ent) + slot * P.ldc;
        const bool mod = is_rel ? P.mod_rel != 0 : P.mod_ent != 0;
        const float cg = is_rel ? P.cg_rel : P.cg_ent;
        if (c == 0) (is_rel ? P.dest_rel : P.dest_ent)[slot] = id;
        double sum = 0.0;
        if (mod) {
            const int half = P.k_int >> 1;
            float a[W], b[W], ga[W], gb[W];
            br_load<W>(row, c, a);
            br_load<W>(row, half + c, b);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                float term;
                br_pair<PW>(a[w], b[w], cg, &ga[w], &gb[w], &term);
                sum += (double)term;
            }
            br_store<W>(out, c, ga);
            br_store<W>(out, half + c, gb);
        } else {
            float x[W], g[W];
            br_load<W>(row, c, x);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                float term;
                g[w] = br_plain<PW>(x[w], cg, &term);
                sum += (double)term;
            }
            br_store<W>(out, c, g);
        }
        part += sum * (double)(is_rel ? P.cv_rel : P.cv_ent);
    }
    block_add_double(P.value, part);
}

template <int W>
void (*br_kernel(int p))(const BatchregParams) {
    switch (p) {
        case 1: return batchreg_kernel<1, W>;
        case 2: return batchreg_kernel<2, W>;
        default: return batchreg_kernel<3, W>;
    }
}

}  // namespace
}  // namespace emg

using namespace emg;

extern "C" int emg_batchreg(const emg_batchreg_args* a, void* stream) {
    EMG_REQUIRE(a, "emg_batchreg: null args");
    EMG_REQUIRE(a->p >= 1 && a->p <= 3, "emg_batchreg: p = %d outside 1..3", (int)a->p);
    EMG_REQUIRE((a->form_ent == EMG_BATCHREG_PLAIN || a->form_ent == EMG_BATCHREG_MODULUS) &&
                (a->form_rel == EMG_BATCHREG_PLAIN || a->form_rel == EMG_BATCHREG_MODULUS), "emg_batchreg: unknown form");
    EMG_REQUIRE(a->B >= 0 && a->k_int > 0, "emg_batchreg: bad sizes (B = %lld, k_int = %d)", (long long)a->B, (int)a->k_int);
    EMG_REQUIRE((a->form_ent != EMG_BATCHREG_MODULUS && a->form_rel != EMG_BATCHREG_MODULUS) || a->k_int % 2 == 0,
                "emg_batchreg: odd k_int in the modulus form");
    EMG_REQUIRE(a->n_ent > 0 && a->n_ent < ((int64_t)1 << 31) && a->n_rel > 0 && a->n_rel < ((int64_t)1 << 31), "emg_batchreg: bad table sizes");
    EMG_REQUIRE(a->ld_ent >= a->k_int && a->ld_rel >= a->k_int, "emg_batchreg: bad strides");
    if (a->B == 0) return EMG_OK;
    const bool has_rel = a->coef_v_rel != 0.f || a->coef_g_rel != 0.f;   // lambda_rel != 0
    EMG_REQUIRE(a->ent && a->pos && a->contrib_ent && a->dest_ent, "emg_batchreg: null pointer");
    EMG_REQUIRE(!has_rel || (a->rel && a->contrib_rel && a->dest_rel), "emg_batchreg: null pointer (relation rows, lambda_rel != 0)");
    EMG_REQUIRE(a->ldc >= a->k_int, "emg_batchreg: ldc < k_int");
    BatchregParams P;
    P.k_int = a->k_int;
    P.mod_ent = a->form_ent == EMG_BATCHREG_MODULUS; P.mod_rel = a->form_rel == EMG_BATCHREG_MODULUS;
    P.cg_ent = a->coef_g_ent; P.cv_ent = a->coef_v_ent; P.cg_rel = a->coef_g_rel; P.cv_rel = a->coef_v_rel;
    P.ent = a->ent; P.n_ent = a->n_ent; P.ld_ent = a->ld_ent; P.rel = a->rel; P.n_rel = a->n_rel; P.ld_rel = a->ld_rel;
    P.pos = a->pos; P.B = a->B;
    P.contrib_ent = a->contrib_ent; P.contrib_rel = a->contrib_rel; P.ldc = a->ldc;
    P.dest_ent = a->dest_ent; P.dest_rel = a->dest_rel; P.value = a->value;
    // 16-byte accesses: every row 16-byte aligned, and groups of four columns that never straddle a row's end or a row's halves
    const int cols_ent = P.mod_ent ? a->k_int / 2 : a->k_int, cols_rel = P.mod_rel ? a->k_int / 2 : a->k_int;
    bool vec = cols_ent % 4 == 0 && a->ld_ent % 4 == 0 && a->ldc % 4 == 0 && aligned16(a->ent) && aligned16(a->contrib_ent);
    if (has_rel) vec = vec && cols_rel % 4 == 0 && a->ld_rel % 4 == 0 && aligned16(a->rel) && aligned16(a->contrib_rel);
    const int W = vec ? 4 : 1;
    P.nq_ent = cols_ent / W;
    P.nq_rel = cols_rel / W;
    P.items_ent = 2 * a->B * P.nq_ent;
    P.items = P.items_ent + (has_rel ? a->B * P.nq_rel : 0);
    const int64_t need = cdiv(P.items, kBrThreads);
    const int64_t blocks = need < kBrMaxGroups ? need : kBrMaxGroups;
    hipStream_t st = (hipStream_t)stream;
    void (*fn)(const BatchregParams) = vec ? br_kernel<4>(a->p) : br_kernel<1>(a->p);
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kBrThreads), 0, st, P);
    EMG_LAUNCH_CHECK();
    // waits for the launch and reports an id the kernel refused
    int32_t bad = 0;
    EMG_HIP(hipMemcpyFromSymbolAsync(&bad, HIP_SYMBOL(g_batchreg_bad), sizeof(bad), 0, hipMemcpyDeviceToHost, st));
    EMG_HIP(hipStreamSynchronize(st));
    if (!bad) return EMG_OK;
    const int32_t zero = 0;
    EMG_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_batchreg_bad), &zero, sizeof(zero), 0, hipMemcpyHostToDevice, st));
    EMG_HIP(hipStreamSynchronize(st));
    return fail(EMG_EINVAL, "emg_batchreg: pos holds an id outside its table");
}
