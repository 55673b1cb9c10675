// the fused training kernels of model 4 with a score link / FocusE edge weights on the scores (emgraph_hip.h: emg_backward_args.link,
// edge_w), a translation unit of its own beside emg_fused_m4.hip (emg_fused_inst.inc)
#define EMG_FUSED_MODEL 4
#define EMG_FUSED_LINKED 1
#define EMG_FUSED_NAME launch_fused_l
#include "emg_fused_inst.inc"
