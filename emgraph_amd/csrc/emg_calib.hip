// emg_calib.hip — Platt-scaling calibration on frozen embeddings (EmbeddingModel.py:2212-2575: _calibrate_with_corruptions,
// _calibrate_with_negatives, _calibrate, _predict_proba; AmpliGraph 1.x's calibrate / predict_proba).
//
// Two scalars (w, b) are fitted to the raw scores: logit x = -(w s + b), loss = sum weight * ce(label, x) / #scores with
// ce(z, x) = max(x, 0) - x z + log1p(exp(-|x|)) (tf.losses.sigmoid_cross_entropy with weights, :2439-2506).
//
//   emg_calib_step     mode 2 (:2212-2260, :2509-2531), one launch per optimiser step: a wave per row of the batch draws the
//                      row's corruption (eta = 1, side 's,o', all entities: corruption_draw, the bits of emg_corrupt_codes), gathers
//                      the negative's three rows and scores them with the chain of emg_score_kernels.hpp (the shape and the lane
//                      assignment emg_score_triples takes for these rows: the same bits), and forms the logistic terms of the
//                      negative and of its positive (whose score the caller computed once: the embeddings are frozen) in double.
//   emg_calib_moments  mode 1 (:2262-2287): loss, gradient and Hessian of the objective over all scores at (w, b) for the host's
//                      Newton iteration.
//   emg_calib_proba    predict_proba (:2564-2570): sigmoid(-(w s + b)).
//
// Reduction, both kernels: no atomics on the sums (same-address double atomics cost ~10 ns each, DESIGN.md 7, and their order
// of arrival would be the order of summation).  Every workgroup writes its partial sums to its own slot of the workspace, fences
// (agent-scope release) and takes a ticket from one counter; the workgroup that draws the last ticket acquires, sums the slots
// in a fixed order (lane l of its first wave: slots l, l + 64, ... ascending; then the butterfly over the lanes), does the tail
// (the Adam update of the device state record / the six outputs) and re-arms the counter for the next launch.  Nothing is read
// by the host, set or allocated between two launches; the counter is zero before the first one (the caller zeroes the workspace
// once).
#include "emg_score_kernels.hpp"

#pragma clang fp contract(off)

namespace emg {

constexpr int kCalibWaves = kThreads / 64;      // rows of a batch per workgroup: a wave each
constexpr int kCalibHeader = 256;               // bytes ahead of the slots: the ticket counter
constexpr int kCalibSlot = 6;                   // doubles per slot (the step uses 3)
constexpr int kMomentItems = 4;                 // scores per thread of the moments kernel

struct CalibParams {
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const float* rel; int64_t ld_rel;
    int32_t k_int; int32_t khalf; int32_t nchunks; float scale;
    const int32_t* pos; int64_t B; const float* scores_pos;
    uint64_t seed; uint64_t counter;
    double label_pos, label_neg, weight_pos, weight_neg;
    double lr, beta1, beta2, eps;
    double* state;                // {w, b, m_w, m_b, v_w, v_b, step, loss_sum}
    uint32_t* ticket; double* slots;
    int32_t* dbg_neg; float* dbg_scores;
};

// the logistic terms of one score s at (w, b): loss weight * ce(z, x), x = -(w s + b); d/dw, d/db; with H: the Hessian's entries
struct LogitTerms { double loss, gw, gb, hww, hwb, hbb; };
__device__ __forceinline__ LogitTerms logit_terms(double s, double w, double b, double z, double weight) {
    const double x = -(w * s + b);
    const double e = exp(-fabs(x));
    const double sig = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    const double ce = fmax(x, 0.0) - x * z + log1p(e);
    const double d = weight * (sig - z);            // weight * dce/dx;  dx/dw = -s, dx/db = -1
    const double h = weight * (e / ((1.0 + e) * (1.0 + e)));   // weight * sig (1 - sig)
    LogitTerms t;
    t.loss = weight * ce; t.gw = -(d * s); t.gb = -d;
    t.hww = h * s * s; t.hwb = h * s; t.hbb = h;
    return t;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The end of both kernels.  part[wave][q]: the waves' partial sums in LDS (written before the call, no barrier yet).  Returns true in
// the first wave of the workgroup that drew the last ticket, total[q] then holding the sums over all workgroups (in every lane).
template <int NQ>
__device__ __forceinline__ bool slots_reduce(double (*part)[kCalibSlot], uint32_t* ticket, double* slots, double* total) {
    __syncthreads();
    if (threadIdx.x == 0) {
        double* mine = slots + (int64_t)blockIdx.x * kCalibSlot;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double t = part[0][q];
#pragma unroll
            for (int w = 1; w < kCalibWaves; ++w) t += part[w][q];
            mine[q] = t;
        }
        // publish: the slot leaves this XCD's L2 before the ticket is taken (release, then the wait, then the counter: the order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t last = t == gridDim.x - 1u ? 1u : 0u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        part[kCalibWaves][0] = last ? 1.0 : 0.0;   // (the row behind the waves' rows: "this workgroup is the last", in the one LDS array)
    }
    __syncthreads();
    if (part[kCalibWaves][0] == 0.0 || threadIdx.x >= 64) return false;
    // (the acquire above dropped this compute unit's L1 lines; these loads go past it all the same)
    const int lane = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double acc = 0.0;
        for (unsigned s = lane; s < gridDim.x; s += 64)
            acc += __hip_atomic_load(slots + (int64_t)s * kCalibSlot + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        total[q] = wave_sum_d(acc);
    }
    if (lane == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
    return true;
}

// the step's tail: loss and gradient of the batch -> Keras Adam (adam.py:45; lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t),
// w -= lr_t m / (sqrt(v) + eps)) on the state record
__device__ __forceinline__ void calib_adam(const CalibParams& P, const double* total) {
    double* st = P.state;
    const double n = 2.0 * (double)P.B;     // scores of the batch: B positives, B negatives
    const double g[2] = {total[0] / n, total[1] / n};
    const double t = st[6] + 1.0;
    const double lr_t = P.lr * sqrt(1.0 - pow(P.beta2, t)) / (1.0 - pow(P.beta1, t));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double m = P.beta1 * st[2 + i] + (1.0 - P.beta1) * g[i];
        const double v = P.beta2 * st[4 + i] + (1.0 - P.beta2) * g[i] * g[i];
        st[i] = st[i] - lr_t * m / (sqrt(v) + P.eps);
        st[2 + i] = m; st[4 + i] = v;
    }
    st[6] = t;
    st[7] += total[2] / n;
}

// FORM: 0 a register-tiled shape <W, NV> at a wave per row, 1 the generic strided kernel's sum (rows wider than the tiled
// shapes), 2 EMG_TRANSE_P — the three paths of emg_score_triples (emg_score.hip: decide_step_form / emg_train_forward)
template <int MODEL, int W, int NV, int FORM>
__global__ __launch_bounds__(kThreads) void calib_step_kernel(const CalibParams P) {
    __shared__ double part[kCalibWaves + 1][kCalibSlot];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t g = (int64_t)blockIdx.x * kCalibWaves + wv;
    const bool active = g < P.B;
    if (!active) g = P.B - 1;   // (the whole wave stays convergent; nothing of it is kept)
    const double w = P.state[0], b = P.state[1];

    uint32_t keep, idx;
    corruption_draw(P.seed, P.counter, (uint64_t)g, (uint64_t)P.n_ent, &keep, &idx);
    keep = (uint32_t)__builtin_amdgcn_readfirstlane((int)keep);
    idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
    const int32_t s = keep ? P.pos[3 * g + 0] : (int32_t)idx;   // protocol.py:643-656: keep_subject -> the object is replaced
    const int32_t p = P.pos[3 * g + 1];
    const int32_t o = keep ? (int32_t)idx : P.pos[3 * g + 2];
    const float* es = P.ent + (int64_t)s * P.ld_ent;
    const float* ep = P.rel + (int64_t)p * P.ld_rel;
    const float* eo = P.ent + (int64_t)o * P.ld_ent;

    float score;
    if constexpr (FORM == 0) {
        using R = Row<MODEL, W, NV>;
        R rs, rp, ro;
        load_row<MODEL, W, NV, 64>(rs, es, lane, P.nchunks, P.khalf);
        load_row<MODEL, W, NV, 64>(rp, ep, lane, P.nchunks, P.khalf);
        load_row<MODEL, W, NV, 64>(ro, eo, lane, P.nchunks, P.khalf);
        score = finalize_score<MODEL>(group_sum<64>(partial_score<MODEL, W, NV>(rs, rp, ro)), P.scale, EMG_SCORE_FINAL);
    } else if constexpr (FORM == 1) {
        const int n = is_complex<MODEL>::value ? P.khalf : P.k_int;
        score = finalize_score<MODEL>(group_sum<64>(strided_partial<MODEL>(es, ep, eo, P.khalf, n, lane)), P.scale, EMG_SCORE_FINAL);
    } else {
        score = -transe_p_norm(es, ep, eo, P.k_int, P.scale, lane, nullptr);
    }
    if (active && lane == 0) {
        if (P.dbg_neg) { P.dbg_neg[3 * g + 0] = s; P.dbg_neg[3 * g + 1] = p; P.dbg_neg[3 * g + 2] = o; }
        if (P.dbg_scores) P.dbg_scores[g] = score;
    }
    if (lane == 0) {
        double acc[3] = {0.0, 0.0, 0.0};
        if (active) {
            const LogitTerms tn = logit_terms((double)score, w, b, P.label_neg, P.weight_neg);
            const LogitTerms tp = logit_terms((double)P.scores_pos[g], w, b, P.label_pos, P.weight_pos);
            acc[0] = tp.gw + tn.gw; acc[1] = tp.gb + tn.gb; acc[2] = tp.loss + tn.loss;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) part[wv][q] = acc[q];
    }
    double total[3];
    if (slots_reduce<3>(part, P.ticket, P.slots, total) && lane == 0) calib_adam(P, total);
}

struct MomentParams {
    const float* sp; int64_t n_pos; const float* sn; int64_t n_neg;
    double w, b, label_pos, label_neg, weight_pos, weight_neg;
    uint32_t* ticket; double* slots; double* out;
};

__global__ __launch_bounds__(kThreads) void calib_moments_kernel(const MomentParams P) {
    __shared__ double part[kCalibWaves + 1][kCalibSlot];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = P.n_pos + P.n_neg;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int it = 0; it < kMomentItems; ++it) {
        const int64_t i = ((int64_t)blockIdx.x * kMomentItems + it) * kThreads + threadIdx.x;
        if (i < n) {
            const bool is_pos = i < P.n_pos;
            const double s = is_pos ? (double)P.sp[i] : (double)P.sn[i - P.n_pos];
            const LogitTerms t = logit_terms(s, P.w, P.b, is_pos ? P.label_pos : P.label_neg, is_pos ? P.weight_pos : P.weight_neg);
            acc[0] += t.loss; acc[1] += t.gw; acc[2] += t.gb; acc[3] += t.hww; acc[4] += t.hwb; acc[5] += t.hbb;
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double v = wave_sum_d(acc[q]);
        if (lane == 0) part[wv][q] = v;
    }
    double total[6];
    if (slots_reduce<6>(part, P.ticket, P.slots, total) && lane == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) P.out[q] = total[q] / (double)n;
    }
}

__global__ __launch_bounds__(256) void calib_proba_kernel(const float* __restrict__ s, int64_t n, double w, double b, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = -(w * (double)s[i] + b);
    const double e = exp(-fabs(x));
    out[i] = (float)(x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e));
}

// the step kernels of a model: the six register-tiled shapes at a wave per row (kShape 2 .. 7 of emg_score.hip; the narrower
// groups of shapes 0 / 1 add zeros in the missing levels of group_sum: the same bits), then the generic form
typedef void (*CalibKernel)(const CalibParams);
struct CalibKernels { CalibKernel tiled[6], generic; };
template <int M>
static constexpr CalibKernels calib_kernels() {
    return {{calib_step_kernel<M, 4, 1, 0>, calib_step_kernel<M, 4, 2, 0>, calib_step_kernel<M, 1, 1, 0>, calib_step_kernel<M, 1, 2, 0>,
             calib_step_kernel<M, 1, 4, 0>, calib_step_kernel<M, 1, 8, 0>}, calib_step_kernel<M, 1, 1, 1>};
}
static const CalibKernels kCalibKernels[5] = {calib_kernels<0>(), calib_kernels<1>(), calib_kernels<2>(), calib_kernels<3>(), calib_kernels<4>()};

static int calib_workspace(void* ws, int64_t ws_bytes, int64_t grid, const char* who, uint32_t** ticket, double** slots) {
    EMG_REQUIRE(ws && aligned16(ws) && ws_bytes >= kCalibHeader + grid * (int64_t)(kCalibSlot * sizeof(double)),
                "%s: the workspace is missing, unaligned or smaller than emg_calib_ws_bytes says", who);
    *ticket = (uint32_t*)ws;
    *slots = (double*)((char*)ws + kCalibHeader);
    return EMG_OK;
}

}  // namespace emg

using namespace emg;

extern "C" int64_t emg_calib_ws_bytes(int64_t n) {
    if (n < 0) return -1;
    return kCalibHeader + cdiv(n, kCalibWaves) * (int64_t)(kCalibSlot * sizeof(double));
}

extern "C" int emg_calib_step(const emg_calib_args* a, void* stream) {
    EMG_REQUIRE(a, "emg_calib_step: null args");
    EMG_REQUIRE(a->B >= 0, "emg_calib_step: negative batch size");
    if (a->B == 0) return EMG_OK;
    EMG_REQUIRE(a->ent && a->rel && a->pos && a->scores_pos && a->state, "emg_calib_step: null pointer");
    EMG_REQUIRE(a->model >= EMG_TRANSE_L1 && a->model <= EMG_TRANSE_P, "emg_calib_step: unknown model id %d", a->model);
    const bool cplx = a->model == EMG_COMPLEX || a->model == EMG_HOLE;
    EMG_REQUIRE(a->k_int > 0 && (!cplx || a->k_int % 2 == 0), "emg_calib_step: bad k_int %d for model %d", a->k_int, a->model);
    EMG_REQUIRE(a->ld_ent >= a->k_int && a->ld_rel >= a->k_int, "emg_calib_step: row stride smaller than k_int");
    EMG_REQUIRE(a->n_ent > 0 && a->n_ent < ((int64_t)1 << 31) && a->n_rel > 0, "emg_calib_step: n_ent=%lld out of range", (long long)a->n_ent);
    EMG_REQUIRE(a->model != EMG_TRANSE_P || a->scale > 0.f, "emg_calib_step: EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive");
    EMG_REQUIRE(a->weight_pos > 0.0 && a->weight_neg > 0.0 && a->lr > 0.0, "emg_calib_step: weights and learning rate must be positive");
    const int64_t grid = cdiv(a->B, kCalibWaves);
    EMG_REQUIRE(grid < ((int64_t)1 << 31), "emg_calib_step: batch too large");
    CalibParams P{};
    int rc = calib_workspace(a->workspace, a->workspace_bytes, grid, "emg_calib_step", &P.ticket, &P.slots);
    if (rc != EMG_OK) return rc;
    P.ent = a->ent; P.n_ent = a->n_ent; P.ld_ent = a->ld_ent; P.rel = a->rel; P.ld_rel = a->ld_rel;
    P.k_int = a->k_int; P.scale = a->scale; P.pos = a->pos; P.B = a->B; P.scores_pos = a->scores_pos;
    P.seed = a->seed; P.counter = a->draw_counter;
    P.label_pos = a->label_pos; P.label_neg = a->label_neg; P.weight_pos = a->weight_pos; P.weight_neg = a->weight_neg;
    P.lr = a->lr; P.beta1 = a->beta1; P.beta2 = a->beta2; P.eps = a->eps;
    P.state = a->state; P.dbg_neg = a->dbg_neg; P.dbg_scores = a->dbg_scores;
    CalibKernel k;
    if (a->model == EMG_TRANSE_P) {
        k = calib_step_kernel<EMG_TRANSE_L1, 1, 1, 2>;
    } else {
        // the shape emg_score_triples scores these rows in (decide_step_form's forward pass)
        const int n = step_columns(a->model, a->k_int);
        const bool vec = (n % 4 == 0) && (a->ld_ent % 4 == 0) && (a->ld_rel % 4 == 0) && aligned16(a->ent) && aligned16(a->rel);
        const int c = vec ? n / 4 : n;
        P.khalf = cplx ? n : 0;
        P.nchunks = c;
        const CalibKernels& K = kCalibKernels[a->model];
        if (vec) k = c <= kWaveChunks ? K.tiled[0] : (c <= kMaxChunks ? K.tiled[1] : K.generic);
        else k = c <= 64 ? K.tiled[2] : (c <= 128 ? K.tiled[3] : (c <= 256 ? K.tiled[4] : (c <= kColumnBlock ? K.tiled[5] : K.generic)));
    }
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_calib_moments(const float* scores_pos, int64_t n_pos, const float* scores_neg, int64_t n_neg, double w, double b,
                                 double label_pos, double label_neg, double weight_pos, double weight_neg, double* out,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    EMG_REQUIRE(n_pos >= 0 && n_neg >= 0 && n_pos + n_neg > 0, "emg_calib_moments: no scores");
    EMG_REQUIRE((scores_pos || n_pos == 0) && (scores_neg || n_neg == 0) && out, "emg_calib_moments: null pointer");
    const int64_t grid = cdiv(n_pos + n_neg, (int64_t)kThreads * kMomentItems);
    EMG_REQUIRE(grid < ((int64_t)1 << 31), "emg_calib_moments: too many scores");
    MomentParams P{};
    int rc = calib_workspace(workspace, workspace_bytes, grid, "emg_calib_moments", &P.ticket, &P.slots);
    if (rc != EMG_OK) return rc;
    P.sp = scores_pos; P.n_pos = n_pos; P.sn = scores_neg; P.n_neg = n_neg; P.w = w; P.b = b;
    P.label_pos = label_pos; P.label_neg = label_neg; P.weight_pos = weight_pos; P.weight_neg = weight_neg; P.out = out;
    hipLaunchKernelGGL(calib_moments_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_calib_proba(const float* scores, int64_t n, float w, float b, float* out, void* stream) {
    EMG_REQUIRE(n >= 0, "emg_calib_proba: negative size");
    if (n == 0) return EMG_OK;
    EMG_REQUIRE(scores && out, "emg_calib_proba: null pointer");
    hipLaunchKernelGGL(calib_proba_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, scores, n, (double)w, (double)b, out);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
