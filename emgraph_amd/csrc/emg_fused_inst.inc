// emg_fused_inst.inc — the fused (rider-carrying) kernels of ONE model: every gradient row to the contribution buffer (ip 0) or singletons in place (1 .. 6: emg_score_kernels.hpp::ip_traits): included by emg_fused_m<model>.hip with
// EMG_FUSED_MODEL, EMG_FUSED_LINKED (0 / 1) and EMG_FUSED_NAME defined; emg_fused_l<model>.hip: the same forms with a score link / FocusE weights on the scores.
#include "emg_score_kernels.hpp"

namespace emg {

constexpr bool kFusedLinked = EMG_FUSED_LINKED;   // (0 / 1 and the launcher's name EMG_FUSED_NAME: set by the including file)
#define EMG_CAT2(a, b) a##b
#define EMG_CAT(a, b) EMG_CAT2(a, b)

template <int W, int NV, int LPG>
static void fused_shape(int ip, unsigned grid, hipStream_t st, const GroupParams& P, const Riders& riders) {
    if constexpr (LPG == 64 && NV == 1) {   // plain SGD in place, the cache-policy form (train_backward_body's CP)
        if (ip == kIpCachePolicy) {
            hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 1, true, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
            return;
        }
    }
    if (ip == 0) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 0, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
    else if (ip == 1) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 1, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
    else if (ip == 2) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 2, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
    else if (ip == 3) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 3, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
    else if constexpr (LPG == 64 && NV == 1) {   // state rows in the rolling window: a wave per group, one 16-byte chunk per lane and half
        if (ip == 4) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 4, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
        else if (ip == 5) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 5, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
        else if (ip == 6) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 6, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
    }
    if constexpr (LPG == 64) {   // SGD + LP under the deferred dense pass: singleton negatives replayed in registers (a wave per group)
        if (ip == 7) hipLaunchKernelGGL((train_fused_riders_kernel<EMG_FUSED_MODEL, W, NV, LPG, 7, false, kFusedLinked>), dim3(grid), dim3(kThreads), 0, st, P, riders);
    }
}

void EMG_CAT(EMG_FUSED_NAME, EMG_FUSED_MODEL)(int shape, int ip, unsigned grid, hipStream_t st, const GroupParams& P,
                                              const Riders& riders) {
    if (shape == 0) fused_shape<4, 1, 16>(ip, grid, st, P, riders);
    else if (shape == 1) fused_shape<4, 1, 32>(ip, grid, st, P, riders);
    else if (shape == 2) fused_shape<4, 1, 64>(ip, grid, st, P, riders);
    else fused_shape<4, 2, 64>(ip, grid, st, P, riders);
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
