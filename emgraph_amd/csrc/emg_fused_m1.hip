// the fused in-place training kernels of model 1 (include/emgraph_hip.h: EMG_TRANSE_L1 .. EMG_HOLE), a translation unit of
// its own so that the five models compile in parallel (emg_fused_inst.inc)
#define EMG_FUSED_MODEL 1
#define EMG_FUSED_LINKED 0
#define EMG_FUSED_NAME launch_fused_m
#include "emg_fused_inst.inc"
