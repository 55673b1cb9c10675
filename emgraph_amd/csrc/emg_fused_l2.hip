// the fused training kernels of model 2 with a score link / FocusE edge weights on the scores (emgraph_hip.h: emg_backward_args.link,
// edge_w), a translation unit of its own beside emg_fused_m2.hip (emg_fused_inst.inc)
#include "emg_fused_inst.inc"
template emg::FusedKernel emg::fused_kernel<2, true>(int, int, bool);
