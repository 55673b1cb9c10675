// emg_fused_inst.inc — the fused (rider-carrying) 16-byte-row kernels of ONE model, with (emg_fused_l<model>.hip) or without
// (emg_fused_m<model>.hip) a score link / FocusE weights on the scores: the lookup fused_kernel<MODEL, LINKED>
// (emg_score_kernels.hpp), which the including file instantiates explicitly — that instantiation is what compiles the kernels.
#include "emg_score_kernels.hpp"

namespace emg {

template <int M, bool L, int NV, int LPG, int IP, bool CP = false>
constexpr FusedKernel kFused = train_fused_riders_kernel<M, 4, NV, LPG, IP, CP, L>;

template <int M, bool L>   // (model, linked)
FusedKernel fused_kernel(int shape, int ip, bool cache_policy) {
    // by shape and in-place form.  Forms 4 .. 6 (state rows in the rolling window) are a wave per group with one chunk per lane,
    // form 7 (SGD + LP, lagging singletons replayed in registers) a wave per group
    static const FusedKernel forms[4][8] = {
        {kFused<M, L, 1, 16, 0>, kFused<M, L, 1, 16, 1>, kFused<M, L, 1, 16, 2>, kFused<M, L, 1, 16, 3>, nullptr, nullptr, nullptr, nullptr},
        {kFused<M, L, 1, 32, 0>, kFused<M, L, 1, 32, 1>, kFused<M, L, 1, 32, 2>, kFused<M, L, 1, 32, 3>, nullptr, nullptr, nullptr, nullptr},
        {kFused<M, L, 1, 64, 0>, kFused<M, L, 1, 64, 1>, kFused<M, L, 1, 64, 2>, kFused<M, L, 1, 64, 3>,
         kFused<M, L, 1, 64, 4>, kFused<M, L, 1, 64, 5>, kFused<M, L, 1, 64, 6>, kFused<M, L, 1, 64, 7>},
        {kFused<M, L, 2, 64, 0>, kFused<M, L, 2, 64, 1>, kFused<M, L, 2, 64, 2>, kFused<M, L, 2, 64, 3>, nullptr, nullptr, nullptr, kFused<M, L, 2, 64, 7>}};
    if (shape < 0 || shape > 3 || ip < 0 || ip > 7) return nullptr;
    // plain SGD in place, the cache-policy form (train_backward_body's CP): one chunk per lane of a wave only
    if (cache_policy) return shape == 2 && ip == IP_SGD ? kFused<M, L, 1, 64, 1, true> : nullptr;
    return forms[shape][ip];
}

}  // namespace emg

#ifdef EMG_TRACE   // (a variant library defines EMG_TRACE for ONE of the fused translation units)
extern "C" int emg_trace_read_fused(unsigned long long* host, int64_t n_words) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(emg::emg_trace_fused_buf), (size_t)n_words * 8) == hipSuccess ? 0 : -1;
}
extern "C" int emg_trace_clear_fused(void) {
    static unsigned long long zeros[4 * 65536];
    return hipMemcpyToSymbol(HIP_SYMBOL(emg::emg_trace_fused_buf), zeros, sizeof(zeros)) == hipSuccess ? 0 : -1;
}
#endif
