// the fused training kernels of model 1 with a score link / FocusE edge weights on the scores (emgraph_hip.h: emg_backward_args.link,
// edge_w), a translation unit of its own beside emg_fused_m1.hip (emg_fused_inst.inc)
#include "emg_fused_inst.inc"
template emg::FusedKernel emg::fused_kernel<1, true>(int, int, bool);
