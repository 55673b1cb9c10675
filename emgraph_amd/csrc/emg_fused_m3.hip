// the fused in-place training kernels of model 3 (include/emgraph_hip.h: EMG_TRANSE_L1 .. EMG_HOLE), a translation unit of
// its own so that the five models compile in parallel (emg_fused_inst.inc)
#include "emg_fused_inst.inc"
template emg::FusedKernel emg::fused_kernel<3, false>(int, int, bool);
