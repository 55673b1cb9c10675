// emg_score.hip — fused embedding gather + score (K1+K2+K4), its adjoint (K7) and the fused train kernel.
//
// Replaces, per training batch, EmbeddingModel._lookup_embeddings (EmbeddingModel.py:490-533, three
// materialised tf.nn.embedding_lookup gathers), Model._fn (TransE.py:208-216, DistMult.py:201,
// ComplEx.py:288-298, HolE.py:189), the positive tiling (EmbeddingModel.py:724-729), Loss.apply for the
// pair-local losses, and the TF-autodiff backward of all of them.
//
// Mapping to CDNA4: one LANE GROUP (16/32/64 lanes of a wave64) owns one positive triple.  The
// group keeps the s, p, o rows in VGPRs (16-byte global_load_dwordx4 per lane, rows are 16-byte
// aligned), scores the positive, then streams the eta replacement rows of that positive — the
// relation row and the kept side are read ONCE per group instead of once per negative:
// (3+eta) row reads per group instead of 3(1+eta).  k-reductions are __shfl_xor butterflies.
//
// Backward/fused kernel: for the pair-local losses (pairwise, nll, absolute_margin) dL/dneg_j depends only
// on (pos_i, neg_j), so score -> loss -> gradient happens in ONE pass over the rows.  A gradient row whose
// destination is hit exactly once in the batch (the common case for uniform negatives) is applied to the
// table IN PLACE from the registers that already hold the row: 1 read + 1 write instead of
// read + contribution write + contribution read + RMW.  Race-free: a singleton destination is, by
// definition, read by no other group of this batch.  All other rows go to the contribution buffer and
// are summed in a fixed order by emg_apply_grouped (no float atomics anywhere).
// HBM-bound by design: algorithmic bytes per group in DESIGN.md §4.
//
// Dispatch: decide_step_form derives the form of a step (StepForm: shape, in-place form, flags, column blocks) from the arguments
// and holds every rule and refusal once; launch_step looks the kernels of that form up (one table here, one lookup per fused
// translation unit) and launches them.  emg_train_backward_form is the same path without the launches.
#include <math.h>
#include <string.h>

#include <atomic>

#include "emg_score_kernels.hpp"

namespace emg {

// ---------------------------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------------------------
enum class Pass { Forward, Backward, Fused };

// The cache-policy form of the fused in-place SGD kernel (train_backward_body's CP) where the rows this step touches twice fit
// the Infinity Cache beside nothing else: the table itself does not fit it (a table that does — C1, C2, C5 — is resident
// anyway), and the rows hit more than once plus the contribution rows, estimated from B, eta and |E| for uniformly drawn rows
// (occupancy: N slots over n rows leave n (1 - (1 - 1/n)^N) distinct rows, N (1 - 1/n)^(N - 1) of them singletons), stay within
// the largest set tools/mall_residency measured fully resident behind a non-temporal stream.  No device read-back: a skewed
// batch (fewer singletons) only makes the true set smaller.  EMG_CACHE_POLICY=0|1 forces the form (tests/test_cache_policy_forms.py).
constexpr double kMallBytes = 256.0 * 1024 * 1024;
constexpr double kResidentBudget = 240e6;
static bool cache_policy_form(const GroupParams& P) {
    const int forced = sw_int(SW_CACHE_POLICY);
    if (forced == 0 || forced == 1) return forced == 1;
    const double n = (double)P.n_ent, row = 4.0 * (double)P.ld_ent;
    if (n < 2 || n * row <= kMallBytes) return false;
    const double N = (double)P.B * (2 + P.eta);
    const double l = log1p(-1.0 / n);
    const double distinct = n * -expm1(N * l), singles = N * exp((N - 1) * l);
    const double multi = distinct > singles ? distinct - singles : 0.0;
    // contribution rows: dE[s], dE[o], dE[p] and (factored) the two query rows; unfactored, one per negative that is no singleton
    const double contrib = 5.0 * (double)P.B + (P.fac.coef ? 0.0 : (N - singles));
    return (multi + contrib) * row <= kResidentBudget;
}

static std::atomic<int64_t> g_cache_policy_launches{0};   // (emg_cache_policy_launches: tests see which form ran)

// The decided form of a training step: what decide_step_form derives from the arguments and launch_step looks up and launches.
enum RidersGo : int32_t { RIDERS_NONE = 0, RIDERS_RIDE = 1, RIDERS_ALONE = 2 };   // carried by the launch / launched alone, first
struct StepForm {
    Pass pass; int32_t model, n;   // n: columns per row (per half for complex models)
    int32_t W, shape;              // floats per chunk (4: 16-byte rows, 1: scalar rows); kShape index of a block, -1: the generic forward kernel
    int32_t ip;                    // InPlace
    bool wave_per_group, cache_policy, linked;
    int32_t riders;                // RidersGo
    int32_t blocks;                // launches of kColumnBlock columns each (1 unless wide-row backward; 0: an empty batch)
};
// {chunks per lane, lanes per group} of the register-tiled shapes: 0 .. 3 16-byte rows (fused_kernel's numbering), 4 .. 7 scalar rows
static const int32_t kShape[8][2] = {{1, 16}, {1, 32}, {1, 64}, {2, 64}, {1, 64}, {2, 64}, {4, 64}, {8, 64}};
static int ladder(bool vec, int c, bool wave_per_group) {   // the shape for rows of c chunks; -1: none holds them
    if (vec) return c <= 16 && !wave_per_group ? 0 : (c <= 32 && !wave_per_group ? 1 : (c <= kWaveChunks ? 2 : (c <= kMaxChunks ? 3 : -1)));
    return c <= 64 ? 4 : (c <= 128 ? 5 : (c <= 256 ? 6 : (c <= kColumnBlock ? 7 : -1)));
}

// Every rule of the dispatch, once: the form of the step, or the refusal.  Reads P and the run-time switches, touches no device.
static int decide_step_form(Pass pass, int model, const GroupParams& P, bool have_riders, StepForm* out) {
    StepForm f{};
    f.pass = pass; f.model = model;
    const int n = f.n = step_columns(model, P.k_int);
    // the forms that replay lagging singletons (emg_backward_args.lr_hist; train_backward_impl has checked the rest of what they ask)
    if (P.lr_hist && P.opt.opt == EMG_OPT_SGD) {   // (form 7)
        EMG_REQUIRE(replay_rows(n, kMaxChunks, P.ld_ent, P.ent),
                    "emg_train_backward_ex: lr_hist needs 16-byte rows of at most %d chunks (per half for complex models)", kMaxChunks);
    } else if (P.lr_hist) {                        // (form 6)
        EMG_REQUIRE(replay_rows(n, kWaveChunks, P.ld_ent, P.ent) && aligned16(P.ent_state0) && aligned16(P.ent_state1) && !P.ctl,
                    "emg_train_backward_ex: lr_hist needs 16-byte rows of at most %d chunks (per half for complex models) and no device-side step record", kWaveChunks);
    }
    const bool cplx = (model == EMG_COMPLEX || model == EMG_HOLE);
    EMG_REQUIRE(model >= 0 && model <= EMG_HOLE, "unknown model id %d", model);
    EMG_REQUIRE(P.k_int > 0 && (!cplx || P.k_int % 2 == 0), "bad k_int %d for model %d", P.k_int, model);
    EMG_REQUIRE(P.ld_ent >= P.k_int && P.ld_rel >= P.k_int, "row stride smaller than k_int");
    EMG_REQUIRE(P.B >= 0 && P.eta >= 0, "negative sizes");
    if (P.B == 0) { *out = f; return EMG_OK; }
    EMG_REQUIRE(P.B * (int64_t)kThreads < ((int64_t)1 << 37), "batch too large");
    // 16-byte rows: whole chunks, every table the pass touches aligned
    bool vec = (n % 4 == 0) && (P.ld_ent % 4 == 0) && (P.ld_rel % 4 == 0) && aligned16(P.ent) && aligned16(P.rel);
    if (pass != Pass::Forward) {
        vec = vec && (P.ldc % 4 == 0) && aligned16(P.contrib_ent) && aligned16(P.contrib_rel);
        if (P.single_ent)
            vec = vec && (!P.ent_state0 || aligned16(P.ent_state0)) && (!P.ent_state1 || aligned16(P.ent_state1));
    }
    f.W = vec ? 4 : 1;
    const bool sgd = P.opt.opt == EMG_OPT_SGD;
    if (pass != Pass::Forward && P.single_ent && sgd && P.opt.lp_lambda != 0.f && !vec)
        return fail(EMG_ENOSUP, "train backward: in-place updates fold an LP regulariser for 16-byte aligned rows only (k, or k per "
                                "half for complex models, a multiple of 4); pass single_ent = NULL");
    if (P.window && !(vec && pass == Pass::Fused && n / 4 <= kWaveChunks && P.single_ent && !sgd))
        return fail(EMG_ENOSUP, "train backward: inplace_window (a stateful optimizer's state rows travelling with the table rows) needs the "
                                "fused kernel on 16-byte aligned rows of at most %d chunks (per half for complex models)", kWaveChunks);
    if (pass == Pass::Forward || !P.single_ent) f.ip = IP_NONE;
    else if (sgd) f.ip = P.opt.lp_lambda == 0.f ? IP_SGD : (P.lr_hist ? IP_SGD_LP_LAG : IP_SGD_LP);   // (lr_hist: under the deferred dense pass)
    else if (!P.window) f.ip = IP_STATE;
    else f.ip = P.lr_hist ? IP_WINDOW_LAG : ((P.opt.opt == EMG_OPT_ADAM || P.opt.opt == EMG_OPT_ADAM_LAZY) ? IP_WINDOW_2 : IP_WINDOW_1);
    // only the fused 16-byte-row kernels carry riders; everything else: the stages alone, first
    f.riders = !have_riders ? RIDERS_NONE : ((pass == Pass::Fused && vec && n <= kColumnBlock) ? RIDERS_RIDE : RIDERS_ALONE);
    // Forms 4 .. 7 are compiled for a wave per group only.  Otherwise narrow rows share a wave (4 / 2 groups of 16 / 32 lanes) unless
    // the batch is too small to put two waves on every SIMD: then a wave per group (idle lanes cost nothing while every wave waits
    // for memory; same bits: the reduction's extra levels add zeros).  EMG_WIDE_GROUPS >= 0 forces either; the forward kernel shares.
    const int wide_env = sw_int(SW_WIDE_GROUPS);
    f.wave_per_group = f.ip >= IP_WINDOW_1 || (pass != Pass::Forward && (wide_env >= 0 ? wide_env != 0 : P.B <= 2048));
    f.blocks = 1; f.shape = ladder(vec, n / f.W, f.wave_per_group);
    if (f.shape < 0 && pass == Pass::Fused)
        return fail(EMG_ENOSUP, "fused score+loss+gradient: rows of k_int=%d are wider than the register-tiled kernel holds "
                                "(512 columns per half) — use emg_train_forward + emg_loss + emg_train_backward_ex(fused_loss = -1), "
                                "which splits wide rows into column blocks", P.k_int);
    if (f.shape < 0 && pass == Pass::Backward) {
        // WIDE rows: given dL/dscore every gradient is separable by column, so the register-tiled kernel runs once per block of 512
        // columns on offset pointers.  TransE-L2's gradient needs the FULL norm: the caller passes the final scores.
        EMG_REQUIRE(model != EMG_TRANSE_L2 || (P.bw_scores_pos && (P.eta == 0 || P.bw_scores_neg)),
                    "train backward: TransE-L2 rows wider than 512 columns need bw_scores_pos / bw_scores_neg (the full norms)");
        f.blocks = (int32_t)cdiv(n, kColumnBlock);
        f.shape = ladder(vec, kColumnBlock / f.W, f.wave_per_group);
    }   // (forward: shape -1, the generic kernel — any width, a wave per group)
    f.linked = pass == Pass::Fused && (P.link != EMG_LINK_LINEAR || P.edge_w);   // the LINKED forms (train_backward_body)
    // the cache-policy form exists for plain SGD in place at one chunk per lane of a wave
    f.cache_policy = pass == Pass::Fused && f.shape == 2 && f.ip == IP_SGD && cache_policy_form(P);
    *out = f;
    return EMG_OK;
}

// The kernels of this translation unit by model and shape: forward; backward from external dL/dscore by in-place form (IP 3, SGD
// folding LP, for 16-byte rows only); for scalar rows the fused forms [linked][in-place form].  nullptr: no such kernel.
struct ShapeKernels { GroupKernel forward, backward[4], fused[2][3]; };
struct ModelKernels { ShapeKernels shape[8]; GroupKernel generic_forward; };
template <int M, int W, int NV, int LPG>
static constexpr ShapeKernels shape_kernels() {
    ShapeKernels s{train_forward_kernel<M, W, NV, LPG>,
                   {train_backward_kernel<M, W, NV, LPG, false, 0>, train_backward_kernel<M, W, NV, LPG, false, 1>, train_backward_kernel<M, W, NV, LPG, false, 2>, nullptr}, {}};
    if constexpr (W == 4) s.backward[3] = train_backward_kernel<M, W, NV, LPG, false, 3>;
    else s = {s.forward, {s.backward[0], s.backward[1], s.backward[2], nullptr},
              {{train_backward_kernel<M, W, NV, LPG, true, 0>, train_backward_kernel<M, W, NV, LPG, true, 1>, train_backward_kernel<M, W, NV, LPG, true, 2>},
               {train_backward_kernel<M, W, NV, LPG, true, 0, true>, train_backward_kernel<M, W, NV, LPG, true, 1, true>, train_backward_kernel<M, W, NV, LPG, true, 2, true>}}};
    return s;
}
template <int M>
static constexpr ModelKernels model_kernels() {
    return {{shape_kernels<M, 4, 1, 16>(), shape_kernels<M, 4, 1, 32>(), shape_kernels<M, 4, 1, 64>(), shape_kernels<M, 4, 2, 64>(),
             shape_kernels<M, 1, 1, 64>(), shape_kernels<M, 1, 2, 64>(), shape_kernels<M, 1, 4, 64>(), shape_kernels<M, 1, 8, 64>()}, train_forward_generic_kernel<M>};
}
static_assert(EMG_TRANSE_L1 == 0 && EMG_HOLE == 4, "the kernel tables are indexed by the model");
static const ModelKernels kModelKernels[5] = {model_kernels<0>(), model_kernels<1>(), model_kernels<2>(), model_kernels<3>(), model_kernels<4>()};
typedef FusedKernel (*FusedLookup)(int shape, int ip, bool cache_policy);
static const FusedLookup kFusedLookup[2][5] = {   // [linked][model]: emg_fused_m<model>.hip, emg_fused_l<model>.hip
    {fused_kernel<0, false>, fused_kernel<1, false>, fused_kernel<2, false>, fused_kernel<3, false>, fused_kernel<4, false>},
    {fused_kernel<0, true>, fused_kernel<1, true>, fused_kernel<2, true>, fused_kernel<3, true>, fused_kernel<4, true>}};
static GroupKernel group_kernel(const StepForm& f, int shape) {
    if (shape < 0) return kModelKernels[f.model].generic_forward;
    const ShapeKernels& s = kModelKernels[f.model].shape[shape];
    if (f.pass == Pass::Forward) return s.forward;
    if (f.pass == Pass::Backward) return f.ip <= IP_SGD_LP ? s.backward[f.ip] : nullptr;
    return f.ip <= IP_STATE ? s.fused[f.linked][f.ip] : nullptr;
}

// Looks the kernels of a decided form up and launches them: the two launch sites of the family (kernels without and with riders).
// A form without a kernel is an error.  dry: everything but the launches (emg_train_backward_form).
static int launch_step(const StepForm& f, GroupParams& P, hipStream_t st, const Riders* riders_in, bool dry) {
    static const Riders no_riders{};
    const int rc = f.riders == RIDERS_ALONE && !dry ? launch_riders_alone(*riders_in, st) : EMG_OK;
    if (rc != EMG_OK) return rc;
    const Riders& riders = f.riders == RIDERS_RIDE && !dry ? *riders_in : no_riders;
    P.khalf = (f.model == EMG_COMPLEX || f.model == EMG_HOLE) ? f.n : 0;
    P.nchunks = f.n / f.W;
    for (int b = 0; b < f.blocks; ++b) {
        GroupParams Q = P;
        int shape = f.shape;
        if (f.blocks > 1) {   // a block of columns on offset pointers; the last one is narrower
            const int c0 = b * kColumnBlock;
            Q.width = f.n - c0 < kColumnBlock ? f.n - c0 : kColumnBlock;
            Q.nchunks = Q.width / f.W;
            shape = ladder(f.W == 4, Q.nchunks, f.wave_per_group);
            Q.ent += c0; Q.rel += c0; Q.contrib_ent += c0; Q.contrib_rel += c0;
            if (Q.ent_rw) Q.ent_rw += c0;
            if (Q.ent_state0) Q.ent_state0 += c0;
            if (Q.ent_state1) Q.ent_state1 += c0;
        }
        const bool with_riders = f.pass == Pass::Fused && f.W == 4;   // (the kernels of the fused translation units)
        const FusedKernel kf = with_riders ? kFusedLookup[f.linked][f.model](shape, f.ip, f.cache_policy) : nullptr;
        const GroupKernel kg = with_riders ? nullptr : group_kernel(f, shape);
        if (!kf && !kg)
            return fail(EMG_ENOSUP, "training step: no kernel for pass %d of model %d, %d-float chunks, shape %d, in-place form %d%s%s", (int)f.pass,
                        f.model, f.W, shape, f.ip, f.cache_policy ? ", cache policy" : "", f.linked ? ", linked" : "");
        if (dry) continue;
        const unsigned grid = (unsigned)cdiv(P.B, kThreads / (shape < 0 ? 64 : kShape[shape][1])) + riders.total;   // (riders.total != 0 only where they ride)
        if (kf && f.cache_policy) g_cache_policy_launches.fetch_add(1);
        if (kf) hipLaunchKernelGGL(kf, dim3(grid), dim3(kThreads), 0, st, Q, riders);
        else hipLaunchKernelGGL(kg, dim3(grid), dim3(kThreads), 0, st, Q);
        EMG_LAUNCH_CHECK();
    }
    return EMG_OK;
}

// decide, then launch what was decided; form_out != nullptr: the dry run (emg_train_backward_form) reports the decision instead
static int run_group_pass(Pass pass, int model, GroupParams& P, hipStream_t st, const Riders* riders = nullptr, bool have_riders = false,
                          int32_t* form_out = nullptr) {
    StepForm f;
    int rc = decide_step_form(pass, model, P, have_riders, &f);
    if (rc == EMG_OK) rc = launch_step(f, P, st, riders, form_out != nullptr);
    if (rc != EMG_OK || !form_out) return rc;
    const int32_t fields[8] = {(int32_t)f.pass, f.model, f.W, f.shape < 0 ? 0 : kShape[f.shape][0], f.shape < 0 ? 64 : kShape[f.shape][1], f.ip,
                               (f.cache_policy ? 1 : 0) | (f.linked ? 2 : 0) | (f.riders << 2), f.blocks};
    memcpy(form_out, fields, sizeof(fields));
    return EMG_OK;
}

__global__ void finalize_scores_kernel(int model, float scale, float* s, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (model == EMG_TRANSE_L2) s[i] = -sqrtf(s[i]);
    else if (model == EMG_HOLE) s[i] = scale * s[i];
}

}  // namespace emg

using namespace emg;

// TransE with any positive order of the norm (EMG_TRANSE_P, `ord` = INFINITY: the largest |component|; TransE.py:208-216
// hands `norm` to tf.norm as ord).  Generic kernels, a wave per triple (inference) or per positive group (training): any
// width, rows read through the caches — orders 1 and 2 are the tuned models, this is the reference's remaining freedom.
//   score      f = -(sum_c |d_c|^ord)^(1/ord),  d = (e_s + e_p) - e_o;  ord = inf: f = -max_c |d_c|
//   gradient   df/dd_c = -sgn(d_c) |d_c|^(ord-1) / ||d||^(ord-1);  ord = inf: -sgn(d_c) [|d_c| = max] / #maxima (tf.reduce_max's
//              gradient is shared by tied maxima); a zero vector has gradient zero
__global__ __launch_bounds__(256) void score_transe_p_kernel(const float* __restrict__ ent, int64_t ld_ent, const float* __restrict__ rel,
                                                             int64_t ld_rel, int k_int, float ord, const int32_t* __restrict__ spo, int64_t n,
                                                             float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (t >= n) return;
    const float nrm = transe_p_norm(ent + (int64_t)spo[3 * t] * ld_ent, rel + (int64_t)spo[3 * t + 1] * ld_rel,
                                    ent + (int64_t)spo[3 * t + 2] * ld_ent, k_int, ord, lane, nullptr);
    if (lane == 0) out[t] = -nrm;
}

struct TransePTrain {
    const float* ent; int64_t ld_ent; const float* rel; int64_t ld_rel; int32_t k_int; float ord;
    const int32_t* pos; int64_t B; int32_t eta; const int32_t* codes;
    float* scores_pos; float* scores_neg;               // forward
    const float* g_pos; const float* g_neg;             // backward: dL/dscore
    float* contrib_ent; float* contrib_rel; int64_t ldc;
};

// scores of a positive and its eta negatives (eta-major codes: replacement | keep_subject << 31)
__global__ __launch_bounds__(256) void transe_p_forward_kernel(const TransePTrain P) {
    const int lane = threadIdx.x & 63;
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (g >= P.B) return;
    const float* es = P.ent + (int64_t)P.pos[3 * g] * P.ld_ent;
    const float* ep = P.rel + (int64_t)P.pos[3 * g + 1] * P.ld_rel;
    const float* eo = P.ent + (int64_t)P.pos[3 * g + 2] * P.ld_ent;
    const float f = -transe_p_norm(es, ep, eo, P.k_int, P.ord, lane, nullptr);
    if (lane == 0) P.scores_pos[g] = f;
    for (int j = 0; j < P.eta; ++j) {
        const int32_t code = P.codes[(int64_t)j * P.B + g];
        const float* er = P.ent + (int64_t)(code & 0x7fffffff) * P.ld_ent;
        const float fn = code < 0 ? -transe_p_norm(es, ep, er, P.k_int, P.ord, lane, nullptr) : -transe_p_norm(er, ep, eo, P.k_int, P.ord, lane, nullptr);
        if (lane == 0) P.scores_neg[(int64_t)j * P.B + g] = fn;
    }
}

// gradient rows of a positive group, in the contribution layout of every model: slot g = dE[s], B + g = dE[o], 2B + jB + g = the
// replacement of negative j, relation slot g = dR[p].  The shared rows accumulate in their slots (the lane that owns a column
// adds to it, positive first, negatives in ascending j: a fixed order).
__global__ __launch_bounds__(256) void transe_p_backward_kernel(const TransePTrain P) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (g >= P.B) return;
    const float* es = P.ent + (int64_t)P.pos[3 * g] * P.ld_ent;
    const float* ep = P.rel + (int64_t)P.pos[3 * g + 1] * P.ld_rel;
    const float* eo = P.ent + (int64_t)P.pos[3 * g + 2] * P.ld_ent;
    float* cs = P.contrib_ent + g * P.ldc;
    float* co = P.contrib_ent + (P.B + g) * P.ldc;
    float* cp = P.contrib_rel + g * P.ldc;
    const bool mx = isinf(P.ord);
    // u_c = -df/dd_c * (-1) ... the triple (a, p, b) with upstream gradient gs gets  da = dp = -gs u,  db = +gs u
    auto unit = [&](float d, float nrm, float ties) -> float {
        const float ad = fabsf(d);
        if (nrm == 0.f || ad == 0.f) return 0.f;
        const float sg = d > 0.f ? 1.f : -1.f;
        if (mx) return ad == nrm ? sg / ties : 0.f;
        return sg * powf(ad, P.ord - 1.f) / powf(nrm, P.ord - 1.f);
    };
    {
        float ties = 1.f;
        const float nrm = transe_p_norm(es, ep, eo, P.k_int, P.ord, lane, &ties);
        const float gs = P.g_pos[g];
        for (int c = lane; c < P.k_int; c += 64) {
            const float v = gs * unit((es[c] + ep[c]) - eo[c], nrm, ties);
            cs[c] = -v; cp[c] = -v; co[c] = v;
        }
    }
    for (int j = 0; j < P.eta; ++j) {
        const int32_t code = P.codes[(int64_t)j * P.B + g];
        const bool keep_s = code < 0;   // subject kept: the OBJECT was replaced
        const float* er = P.ent + (int64_t)(code & 0x7fffffff) * P.ld_ent;
        const float* a = keep_s ? es : er;
        const float* b = keep_s ? er : eo;
        float* cr = P.contrib_ent + (2 * P.B + (int64_t)j * P.B + g) * P.ldc;
        float ties = 1.f;
        const float nrm = transe_p_norm(a, ep, b, P.k_int, P.ord, lane, &ties);
        const float gs = P.g_neg[(int64_t)j * P.B + g];
        for (int c = lane; c < P.k_int; c += 64) {
            const float v = gs * unit((a[c] + ep[c]) - b[c], nrm, ties);
            cp[c] = cp[c] - v;
            if (keep_s) { cs[c] = cs[c] - v; cr[c] = v; }
            else { co[c] = co[c] + v; cr[c] = -v; }
        }
    }
}

static int transe_p_check(int32_t k_int, float ord, int64_t ld_ent, int64_t ld_rel) {
    EMG_REQUIRE(ord > 0.f && k_int > 0 && ld_ent >= k_int && ld_rel >= k_int, "EMG_TRANSE_P: the order of the norm (passed as `scale`) must be positive");
    return EMG_OK;
}

// RotatE (EMG_ROTATE; include/emgraph_hip.h has the contract): f = -sum_j |a_j r_j - b_j| over the k = k_int / 2 complex coordinates,
// r_j = cos(theta_j) + i sin(theta_j) from the first k columns of the relation row.  Generic kernels of the shape of EMG_TRANSE_P's: a
// wave per triple (inference) or per positive group (training), lane l owns coordinates l, l + 64, ...; any width, rows read through
// the caches.  The group kernels take sincosf of the relation row ONCE: a lane keeps (cos, sin) of its coordinates in LDS (it reads
// back only what it wrote itself: no barrier) for the positive and the eta negatives; coordinates from kRotCached on are taken
// again per triple (same function, same bits).
constexpr int kRotCached = 512;
struct RotCoord { float wr, wi, dr, di, m; };
// one coordinate of the triple (a, r, b): w = a r, d = w - b, m = |d| — explicit operations, the same bits in every kernel below
__device__ __forceinline__ RotCoord rotate_coord(float ar, float ai, float cs, float sn, float br, float bi) {
    RotCoord c;
    c.wr = __fmaf_rn(ar, cs, -__fmul_rn(ai, sn));
    c.wi = __fmaf_rn(ar, sn, __fmul_rn(ai, cs));
    c.dr = __fsub_rn(c.wr, br);
    c.di = __fsub_rn(c.wi, bi);
    c.m = sqrtf(__fmaf_rn(c.dr, c.dr, __fmul_rn(c.di, c.di)));
    return c;
}
// (cos, sin) of coordinate j of the relation row `th`: from the wave's cache below kRotCached (cs_w != nullptr), else computed
__device__ __forceinline__ void rotate_phase(const float* th, const float* cs_w, int j, float* cs, float* sn) {
    if (cs_w && j < kRotCached) { *cs = cs_w[j]; *sn = cs_w[kRotCached + j]; }
    else sincosf(th[j], sn, cs);
}
// the wave's sum of moduli of (a, r, b); the score is its negative
__device__ __forceinline__ float rotate_dist(const float* a, const float* th, const float* cs_w, const float* b, int half, int lane) {
    float acc = 0.f;
    for (int j = lane; j < half; j += 64) {
        float cs, sn;
        rotate_phase(th, cs_w, j, &cs, &sn);
        acc = __fadd_rn(acc, rotate_coord(a[j], a[half + j], cs, sn, b[j], b[half + j]).m);
    }
    return wave_sum_f(acc);
}

__global__ __launch_bounds__(256) void score_rotate_kernel(const float* __restrict__ ent, int64_t ld_ent, const float* __restrict__ rel,
                                                           int64_t ld_rel, int k_int, const int32_t* __restrict__ spo, int64_t n,
                                                           float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (t >= n) return;
    const float d = rotate_dist(ent + (int64_t)spo[3 * t] * ld_ent, rel + (int64_t)spo[3 * t + 1] * ld_rel, nullptr,
                                ent + (int64_t)spo[3 * t + 2] * ld_ent, k_int >> 1, lane);
    if (lane == 0) out[t] = -d;
}

// (cos, sin) of the group's relation row into the wave's cache; lane l fills — and later reads — coordinates l, l + 64, ...
__device__ __forceinline__ void rotate_fill_phases(const float* th, float* cs_w, int half, int lane) {
    for (int j = lane; j < half && j < kRotCached; j += 64) sincosf(th[j], &cs_w[kRotCached + j], &cs_w[j]);
}

// scores of a positive and its eta negatives (eta-major codes: replacement | keep_subject << 31); TransePTrain without `ord`
__global__ __launch_bounds__(256) void rotate_forward_kernel(const TransePTrain P) {
    __shared__ float cs_s[4][2 * kRotCached];
    const int lane = threadIdx.x & 63;
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (g >= P.B) return;   // (no workgroup barrier below)
    const int half = P.k_int >> 1;
    const float* es = P.ent + (int64_t)P.pos[3 * g] * P.ld_ent;
    const float* ep = P.rel + (int64_t)P.pos[3 * g + 1] * P.ld_rel;
    const float* eo = P.ent + (int64_t)P.pos[3 * g + 2] * P.ld_ent;
    float* cs_w = cs_s[threadIdx.x >> 6];
    rotate_fill_phases(ep, cs_w, half, lane);
    const float f = -rotate_dist(es, ep, cs_w, eo, half, lane);
    if (lane == 0) P.scores_pos[g] = f;
    for (int j = 0; j < P.eta; ++j) {
        const int32_t code = P.codes[(int64_t)j * P.B + g];
        const float* er = P.ent + (int64_t)(code & 0x7fffffff) * P.ld_ent;
        const float fn = code < 0 ? -rotate_dist(es, ep, cs_w, er, half, lane) : -rotate_dist(er, ep, cs_w, eo, half, lane);
        if (lane == 0) P.scores_neg[(int64_t)j * P.B + g] = fn;
    }
}

// gradient rows of a positive group in the contribution layout of every model (transe_p_backward_kernel): slot g = dE[s], B + g =
// dE[o], 2B + jB + g = the replacement of negative j, relation slot g = dR[p] (phases in columns [0, k), zeros in [k, 2k)).  Every slot
// is written; the shared rows accumulate in their slots, positive first, negatives in ascending j, by the lane that owns the column.
//   u = d / |d| (0 where |d| = 0);  a: -g u conj(r);  b: +g u;  theta: g (u_re w_im - u_im w_re)
__global__ __launch_bounds__(256) void rotate_backward_kernel(const TransePTrain P) {
#pragma clang fp contract(off)
    __shared__ float cs_s[4][2 * kRotCached];
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
    float* cs_w = cs_s[threadIdx.x >> 6];
    rotate_fill_phases(ep, cs_w, half, lane);
    // gradient of coordinate c of the triple (a, p, b) under the upstream gradient gs: ga (2), gb (2), gt
    auto grads = [&](const float* a, const float* b, int c, float gs, float (&ga)[2], float (&gb)[2], float* gt) {
        float cn, sn;
        rotate_phase(ep, cs_w, c, &cn, &sn);
        const RotCoord r = rotate_coord(a[c], a[half + c], cn, sn, b[c], b[half + c]);
        const float ur = r.m > 0.f ? r.dr / r.m : 0.f, ui = r.m > 0.f ? r.di / r.m : 0.f;
        ga[0] = -gs * (ur * cn + ui * sn); ga[1] = -gs * (ui * cn - ur * sn);
        gb[0] = gs * ur; gb[1] = gs * ui;
        *gt = gs * (ur * r.wi - ui * r.wr);
    };
    {
        const float gs = P.g_pos[g];
        for (int c = lane; c < half; c += 64) {
            float ga[2], gb[2], gt;
            grads(es, eo, c, gs, ga, gb, &gt);
            cs[c] = ga[0]; cs[half + c] = ga[1];
            co[c] = gb[0]; co[half + c] = gb[1];
            cp[c] = gt; cp[half + c] = 0.f;
        }
    }
    for (int j = 0; j < P.eta; ++j) {
        const int32_t code = P.codes[(int64_t)j * P.B + g];
        const bool keep_s = code < 0;   // subject kept: the OBJECT was replaced
        const float* er = P.ent + (int64_t)(code & 0x7fffffff) * P.ld_ent;
        const float* a = keep_s ? es : er;
        const float* b = keep_s ? er : eo;
        float* cr = P.contrib_ent + (2 * P.B + (int64_t)j * P.B + g) * P.ldc;
        const float gs = P.g_neg[(int64_t)j * P.B + g];
        for (int c = lane; c < half; c += 64) {
            float ga[2], gb[2], gt;
            grads(a, b, c, gs, ga, gb, &gt);
            cp[c] = cp[c] + gt;
            if (keep_s) {
                cs[c] = cs[c] + ga[0]; cs[half + c] = cs[half + c] + ga[1];
                cr[c] = gb[0]; cr[half + c] = gb[1];
            } else {
                co[c] = co[c] + gb[0]; co[half + c] = co[half + c] + gb[1];
                cr[c] = ga[0]; cr[half + c] = ga[1];
            }
        }
    }
}

static int rotate_check(int32_t k_int, int64_t ld_ent, int64_t ld_rel) {
    EMG_REQUIRE(k_int > 0 && k_int % 2 == 0 && ld_ent >= k_int && ld_rel >= k_int,
                "EMG_ROTATE: k_int = %d must be even (rows [re | im]; the relation row holds k_int / 2 phases) and no wider than the row strides", (int)k_int);
    return EMG_OK;
}

extern "C" int emg_train_forward(int model, const float* ent, int64_t n_ent, int64_t ld_ent, const float* rel,
                                 int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale, const int32_t* pos,
                                 int64_t B, int32_t eta, const int32_t* codes, int32_t flags, float* scores_pos,
                                 float* scores_neg, void* stream) {
    if (B == 0) return EMG_OK;
    EMG_REQUIRE(ent && rel && pos && scores_pos, "emg_train_forward: null pointer");
    if (model == EMG_TRANSE_P) {
        int rc = transe_p_check(k_int, scale, ld_ent, ld_rel);
        if (rc != EMG_OK) return rc;
        EMG_REQUIRE(flags == EMG_SCORE_FINAL, "EMG_TRANSE_P: no partial (column-slab) scores");
        if (eta == 0) {
            hipLaunchKernelGGL(score_transe_p_kernel, dim3((unsigned)cdiv(B * 64, 256)), dim3(256), 0, (hipStream_t)stream, ent, ld_ent, rel, ld_rel,
                               (int)k_int, scale, pos, B, scores_pos);
        } else {
            EMG_REQUIRE(codes && scores_neg, "emg_train_forward: eta>0 needs codes and scores_neg");
            TransePTrain T{};
            T.ent = ent; T.ld_ent = ld_ent; T.rel = rel; T.ld_rel = ld_rel; T.k_int = k_int; T.ord = scale; T.pos = pos; T.B = B; T.eta = eta;
            T.codes = codes; T.scores_pos = scores_pos; T.scores_neg = scores_neg;
            hipLaunchKernelGGL(transe_p_forward_kernel, dim3((unsigned)cdiv(B * 64, 256)), dim3(256), 0, (hipStream_t)stream, T);
        }
        EMG_LAUNCH_CHECK();
        return EMG_OK;
    }
    if (model == EMG_ROTATE) {
        int rc = rotate_check(k_int, ld_ent, ld_rel);
        if (rc != EMG_OK) return rc;
        EMG_REQUIRE(flags == EMG_SCORE_FINAL, "EMG_ROTATE: no partial (column-slab) scores");
        if (eta == 0) {
            hipLaunchKernelGGL(score_rotate_kernel, dim3((unsigned)cdiv(B * 64, 256)), dim3(256), 0, (hipStream_t)stream, ent, ld_ent, rel, ld_rel,
                               (int)k_int, pos, B, scores_pos);
        } else {
            EMG_REQUIRE(codes && scores_neg, "emg_train_forward: eta>0 needs codes and scores_neg");
            TransePTrain T{};
            T.ent = ent; T.ld_ent = ld_ent; T.rel = rel; T.ld_rel = ld_rel; T.k_int = k_int; T.pos = pos; T.B = B; T.eta = eta;
            T.codes = codes; T.scores_pos = scores_pos; T.scores_neg = scores_neg;
            hipLaunchKernelGGL(rotate_forward_kernel, dim3((unsigned)cdiv(B * 64, 256)), dim3(256), 0, (hipStream_t)stream, T);
        }
        EMG_LAUNCH_CHECK();
        return EMG_OK;
    }
    if (model == EMG_SIMPLE)   // the generic kernels of emg_simple.hip
        return simple_forward(ent, ld_ent, rel, ld_rel, k_int, scale, pos, B, eta, codes, flags, scores_pos, scores_neg, stream);
    EMG_REQUIRE(eta == 0 || (codes && scores_neg), "emg_train_forward: eta>0 needs codes and scores_neg");
    GroupParams P{};
    P.ent = ent; P.n_ent = n_ent; P.ld_ent = ld_ent; P.rel = rel; P.n_rel = n_rel; P.ld_rel = ld_rel;
    P.k_int = k_int; P.scale = scale; P.pos = pos; P.B = B; P.eta = eta; P.codes = codes; P.flags = flags;
    P.scores_pos = scores_pos; P.scores_neg = scores_neg;
    return run_group_pass(Pass::Forward, model, P, (hipStream_t)stream);
}

extern "C" int emg_score_triples(int model, const float* ent, int64_t n_ent, int64_t ld_ent, const float* rel,
                                 int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale, const int32_t* spo,
                                 int64_t n, int32_t flags, float* out, void* stream) {
    return emg_train_forward(model, ent, n_ent, ld_ent, rel, n_rel, ld_rel, k_int, scale, spo, n, 0, nullptr, flags,
                             out, nullptr, stream);
}

extern "C" int emg_build_dest(const int32_t* pos, int64_t B, int32_t eta, const int32_t* codes, int32_t* dest_ent,
                              int32_t* dest_rel, void* stream) {
    if (B <= 0) return EMG_OK;
    EMG_REQUIRE(pos && dest_ent && dest_rel && (eta == 0 || codes), "emg_build_dest: null pointer");
    const int64_t n = B * (int64_t)(eta > 1 ? eta : 1);
    hipLaunchKernelGGL(build_dest_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pos, B,
                       (int)eta, codes, dest_ent, dest_rel);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

namespace emg {
int train_backward_impl(const emg_backward_args* a, const Riders* riders, void* stream);
static int backward_step(const emg_backward_args* a, const Riders* riders, bool have_riders, void* stream, int32_t* form_out);
}
extern "C" int emg_train_backward_ex(const emg_backward_args* a, void* stream) { return emg::train_backward_impl(a, nullptr, stream); }
// the dry run: the checks and the decision of emg_train_backward_ex for these arguments, nothing launched, no pointer followed
extern "C" int emg_train_backward_form(const emg_backward_args* a, int32_t have_riders, int32_t out[8]) {
    EMG_REQUIRE(out, "emg_train_backward_form: null out");
    memset(out, 0, 8 * sizeof(int32_t));
    const int rc = emg::backward_step(a, nullptr, have_riders != 0, nullptr, out);
    if (rc != EMG_OK) memset(out, 0, 8 * sizeof(int32_t));
    return rc;
}

// riders (optional): preparation stages of later batches carried by this launch; a pass that cannot carry them (column
// blocks of wide rows, B == 0) launches them on their own first
int emg::train_backward_impl(const emg_backward_args* a, const Riders* riders, void* stream) {
    return backward_step(a, riders, riders && riders->total, stream, nullptr);
}

// form_out != nullptr: the dry run — everything up to the launches, which are left out
static int emg::backward_step(const emg_backward_args* a, const Riders* riders, bool have_riders, void* stream, int32_t* form_out) {
    EMG_REQUIRE(a, "emg_train_backward_ex: null args");
    if (form_out) form_out[6] = have_riders ? RIDERS_ALONE << 2 : 0;   // (the two early exits below: no scoring launch, riders alone)
    if (a->B == 0) return have_riders && !form_out ? launch_riders_alone(*riders, (hipStream_t)stream) : EMG_OK;
    EMG_REQUIRE(a->ent && a->rel && a->pos && a->contrib_ent && a->contrib_rel, "emg_train_backward_ex: null pointer");
    EMG_REQUIRE(a->eta == 0 || a->codes, "emg_train_backward_ex: eta>0 needs codes");
    EMG_REQUIRE(a->ldc >= a->k_int, "emg_train_backward_ex: ldc < k_int");
    const bool fused = a->fused_loss >= 0;
    if (fused) {
        EMG_REQUIRE(a->fused_loss == EMG_LOSS_PAIRWISE || a->fused_loss == EMG_LOSS_NLL ||
                        a->fused_loss == EMG_LOSS_ABSOLUTE_MARGIN,
                    "emg_train_backward_ex: loss %d is not pair-local, use emg_train_forward + emg_loss", a->fused_loss);
        EMG_REQUIRE(a->loss_accum, "emg_train_backward_ex: fused loss needs loss_accum");
        EMG_REQUIRE(!a->bw_scores_pos && !a->bw_scores_neg, "emg_train_backward_ex: fused loss cannot take bw_scores");
        EMG_REQUIRE(a->link >= EMG_LINK_LINEAR && a->link <= EMG_LINK_SOFTPLUS, "emg_train_backward_ex: unknown link %d", a->link);
    } else {
        EMG_REQUIRE(a->link == EMG_LINK_LINEAR && !a->edge_w, "emg_train_backward_ex: a score link / edge weights with external dL/dscore "
                                                              "go through emg_link_scores and emg_link_grads around emg_loss");
        EMG_REQUIRE(a->g_pos && (a->eta == 0 || a->g_neg), "emg_train_backward_ex: external dL/dscore missing");
    }
    if (a->model == EMG_TRANSE_P || a->model == EMG_ROTATE) {   // the generic models: generic kernels, external dL/dscore, every row through the apply
        const bool rot = a->model == EMG_ROTATE;
        EMG_REQUIRE(!fused && !a->single_ent && !a->fac_ws_ent && !a->ctl,
                    "emg_train_backward_ex: %s trains through emg_train_forward + emg_loss + this call with fused_loss = -1, "
                    "without in-place updates, factored contributions or device-side step records", rot ? "EMG_ROTATE" : "EMG_TRANSE_P");
        int rc = rot ? rotate_check(a->k_int, a->ld_ent, a->ld_rel) : transe_p_check(a->k_int, a->scale, a->ld_ent, a->ld_rel);
        if (rc == EMG_OK && form_out) { form_out[0] = (int32_t)Pass::Backward; form_out[1] = a->model; return rc; }
        if (rc == EMG_OK && have_riders) rc = launch_riders_alone(*riders, (hipStream_t)stream);
        if (rc != EMG_OK) return rc;
        TransePTrain T{};
        T.ent = a->ent; T.ld_ent = a->ld_ent; T.rel = a->rel; T.ld_rel = a->ld_rel; T.k_int = a->k_int; T.ord = a->scale; T.pos = a->pos;
        T.B = a->B; T.eta = a->eta; T.codes = a->codes; T.g_pos = a->g_pos; T.g_neg = a->g_neg;
        T.contrib_ent = a->contrib_ent; T.contrib_rel = a->contrib_rel; T.ldc = a->ldc;
        hipLaunchKernelGGL(rot ? rotate_backward_kernel : transe_p_backward_kernel, dim3((unsigned)cdiv(a->B * 64, 256)), dim3(256), 0, (hipStream_t)stream, T);
        EMG_LAUNCH_CHECK();
        return EMG_OK;
    }
    if (a->model == EMG_SIMPLE) {   // a generic model as the two above; its kernel is in emg_simple.hip
        EMG_REQUIRE(!fused && !a->single_ent && !a->fac_ws_ent && !a->ctl,
                    "emg_train_backward_ex: EMG_SIMPLE trains through emg_train_forward + emg_loss + this call with fused_loss = -1, "
                    "without in-place updates, factored contributions or device-side step records");
        int rc = simple_check(a->k_int, a->ld_ent, a->ld_rel);
        if (rc == EMG_OK && form_out) { form_out[0] = (int32_t)Pass::Backward; form_out[1] = a->model; return rc; }
        if (rc == EMG_OK && have_riders) rc = launch_riders_alone(*riders, (hipStream_t)stream);
        return rc != EMG_OK ? rc : simple_backward(a, stream);
    }
    GroupParams P{};
    P.ent = a->ent; P.n_ent = a->n_ent; P.ld_ent = a->ld_ent; P.rel = a->rel; P.n_rel = a->n_rel; P.ld_rel = a->ld_rel;
    P.k_int = a->k_int; P.scale = a->scale; P.pos = a->pos; P.B = a->B; P.eta = a->eta; P.codes = a->codes;
    P.g_pos = a->g_pos; P.g_neg = a->g_neg; P.bw_scores_pos = a->bw_scores_pos; P.bw_scores_neg = a->bw_scores_neg;
    P.fused_loss = a->fused_loss; P.margin = a->margin; P.loss_accum = a->loss_accum;
    P.link = a->link; P.sw = a->sw; P.edge_w = a->edge_w;
    EMG_REQUIRE(a->loss_slots >= 0 && a->loss_slots <= 4096 && (a->loss_slots & (a->loss_slots - 1)) == 0,
                "emg_train_backward_ex: loss_slots must be 0 or a power of two <= 4096");
    P.loss_mask = a->loss_slots > 1 ? (uint32_t)a->loss_slots - 1u : 0u;
    P.scores_pos = a->scores_pos_out; P.scores_neg = a->scores_neg_out;
    P.contrib_ent = a->contrib_ent; P.contrib_rel = a->contrib_rel; P.ldc = a->ldc;
    if (a->fac_ws_ent) {
        EMG_REQUIRE(!(a->model == EMG_TRANSE_L1 || a->model == EMG_TRANSE_L2),
                    "emg_train_backward_ex: factored contributions need a bilinear model — a TransE gradient row depends "
                    "on the replacement entity");
        const int64_t Bl = a->layout_B > 0 ? a->layout_B : a->B;
        int rc = factor_view(a->fac_ws_ent, a->fac_ws_ent_bytes, (2 + (int64_t)a->eta) * Bl, a->n_ent, &P.fac);
        if (rc != EMG_OK) return rc;
    }
    P.single_ent = a->single_ent;
    P.window = a->single_ent && a->inplace_window ? 1 : 0;
    if (a->single_ent) {
        EMG_REQUIRE(a->opt >= EMG_OPT_SGD && a->opt <= EMG_OPT_ADAM_LAZY, "emg_train_backward_ex: unknown optimizer");
        EMG_REQUIRE(!(a->opt == EMG_OPT_MOMENTUM || a->opt == EMG_OPT_ADAGRAD) || a->ent_state0,
                    "emg_train_backward_ex: optimizer needs ent_state0");
        EMG_REQUIRE(!(a->opt == EMG_OPT_ADAM || a->opt == EMG_OPT_ADAM_LAZY) || (a->ent_state0 && a->ent_state1),
                    "emg_train_backward_ex: adam needs both state tables");
        P.ent_rw = const_cast<float*>(a->ent);
        P.ent_state0 = a->ent_state0; P.ent_state1 = a->ent_state1; P.tag_ent = a->tag_ent; P.step = a->step;
        P.opt = make_opt_params(a->opt, a->hyper);
        // A folded LP regulariser (hyper[6] = lambda, hyper[7] = p): plain SGD has its own in-place form (IP 3: the pow / sign
        // code stays out of the other forms, where it costs the fused kernel a wave per SIMD); with a stateful optimizer every
        // gradient row goes through emg_apply_grouped, which folds it in
        if (a->hyper[6] != 0.f) {
            EMG_REQUIRE(a->opt == EMG_OPT_SGD, "emg_train_backward_ex: in-place singleton updates fold an LP regulariser for plain SGD "
                                               "only (pass single_ent = NULL and let emg_apply_grouped apply every row)");
            EMG_REQUIRE(a->lp_accum && a->hyper[7] >= 1.f && a->hyper[7] <= 3.f && a->tag_ent,
                        "emg_train_backward_ex: a folded LP regulariser with in-place updates needs lp_accum, p in {1, 2, 3} and the tag array");
            P.opt.lp_lambda = a->hyper[6]; P.opt.lp_p = (int)a->hyper[7];
            P.lp_accum = a->lp_accum;
        }
    }
    if (a->lr_hist && a->opt == EMG_OPT_SGD) {   // SGD + LP under the deferred dense pass: lagging singleton negatives replayed in the kernel (ip 7)
        EMG_REQUIRE(a->single_ent && !a->inplace_window && a->hyper[6] != 0.f && a->tag_ent && fused && a->step >= 1 && !a->ctl,
                    "emg_train_backward_ex: lr_hist with EMG_OPT_SGD is for the fused kernel with in-place updates and a folded LP regulariser");
        P.lr_hist = a->lr_hist; P.upto = a->step - 1;   // (the rows it fits: decide_step_form)
    } else if (a->lr_hist) {   // Adam's dense pass is deferred: singletons among the negatives lag and are replayed in the kernel (ip 6)
        EMG_REQUIRE(a->single_ent && a->inplace_window && a->opt == EMG_OPT_ADAM && a->hyper[6] == 0.f && a->tag_ent && fused && a->step >= 1,
                    "emg_train_backward_ex: lr_hist (lagging singletons) is for the fused kernel with in-place EMG_OPT_ADAM updates, no regulariser");
        P.lr_hist = a->lr_hist; P.upto = a->step - 1;
    }
    EMG_REQUIRE(a->layout_B == 0 || a->layout_B >= a->B, "emg_train_backward_ex: layout_B < B");
    P.ctl = (const StepCtl*)a->ctl;
    if (P.ctl) {   // the launch covers the capacity; the kernel reads the batch's rows and size from the record
        EMG_REQUIRE(a->layout_B > 0, "emg_train_backward_ex: a device-side step record needs layout_B (the launch size)");
        P.B = a->layout_B;
    }
    return run_group_pass(fused ? Pass::Fused : Pass::Backward, a->model, P, (hipStream_t)stream, riders, have_riders, form_out);
}

extern "C" int emg_train_backward(int model, const float* ent, int64_t n_ent, int64_t ld_ent, const float* rel,
                                  int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale, const int32_t* pos,
                                  int64_t B, int32_t eta, const int32_t* codes, const float* g_pos,
                                  const float* g_neg, float* contrib_ent, float* contrib_rel, int64_t ldc,
                                  int32_t* dest_ent, int32_t* dest_rel, void* stream) {
    if (B == 0) return EMG_OK;
    EMG_REQUIRE(dest_ent && dest_rel, "emg_train_backward: null pointer");
    emg_backward_args a{};
    a.model = model; a.ent = ent; a.n_ent = n_ent; a.ld_ent = ld_ent; a.rel = rel; a.n_rel = n_rel; a.ld_rel = ld_rel;
    a.k_int = k_int; a.scale = scale; a.pos = pos; a.B = B; a.eta = eta; a.codes = codes; a.fused_loss = -1;
    a.g_pos = g_pos; a.g_neg = g_neg; a.contrib_ent = contrib_ent; a.contrib_rel = contrib_rel; a.ldc = ldc;
    int rc = emg_train_backward_ex(&a, stream);
    if (rc != EMG_OK) return rc;
    return emg_build_dest(pos, B, eta, codes, dest_ent, dest_rel, stream);
}

extern "C" int emg_finalize_scores(int model, float scale, float* scores, int64_t n, void* stream) {
    EMG_REQUIRE(scores || n == 0, "emg_finalize_scores: null pointer");
    if (n == 0 || !(model == EMG_TRANSE_L2 || model == EMG_HOLE)) return EMG_OK;
    hipLaunchKernelGGL(finalize_scores_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, model,
                       scale, scores, n);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int64_t emg_cache_policy_launches(void) { return emg::g_cache_policy_launches.load(); }
