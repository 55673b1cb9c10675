"""ctypes binding of libemgraph_hip.so (include/emgraph_hip.h).

The HIP library IS the product's compute path.  There is no CPU fallback: if the shared object is
missing or a call fails this module raises, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _switches

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = _switches.get("EMGRAPH_HIP_LIB") or os.path.join(_HERE, "lib", "libemgraph_hip.so")

# ---- constants mirrored from include/emgraph_hip.h -------------------------------------------
ABI_VERSION = 9
TRANSE_L1, TRANSE_L2, DISTMULT, COMPLEX, HOLE, TRANSE_P, ROTATE = range(7)
SIMPLE = 8   # (7 is unassigned on purpose: the id that names no model)
SIDE_S, SIDE_O, SIDE_SO = range(3)
LOSS_PAIRWISE, LOSS_NLL, LOSS_ABSOLUTE_MARGIN, LOSS_SELF_ADVERSARIAL, LOSS_MULTICLASS_NLL = range(5)
OPT_SGD, OPT_MOMENTUM, OPT_ADAGRAD, OPT_ADAM, OPT_ADAM_LAZY = range(5)
SCORE_FINAL, SCORE_PARTIAL = 0, 1
LINK_LINEAR, LINK_TANH, LINK_SIGMOID, LINK_SOFTPLUS = range(4)
EVAL_S, EVAL_O, EVAL_SPO, EVAL_S_O = range(4)
TOPN_MAX = 128   # EMG_TOPN_MAX
GRID_THR_MAX = 256   # EMG_GRID_THR_MAX

LOSS_IDS = {"pairwise": LOSS_PAIRWISE, "nll": LOSS_NLL, "absolute_margin": LOSS_ABSOLUTE_MARGIN,
            "self_adversarial": LOSS_SELF_ADVERSARIAL, "multiclass_nll": LOSS_MULTICLASS_NLL}
OPT_IDS = {"sgd": OPT_SGD, "momentum": OPT_MOMENTUM, "adagrad": OPT_ADAGRAD, "adam": OPT_ADAM,
           "adam_lazy": OPT_ADAM_LAZY}
LINK_IDS = {"linear": LINK_LINEAR, "tanh": LINK_TANH, "sigmoid": LINK_SIGMOID, "softplus": LINK_SOFTPLUS}
SIDE_IDS = {"s": SIDE_S, "o": SIDE_O, "s+o": SIDE_SO, "s,o": SIDE_SO}
EVAL_SIDE_IDS = {"s": EVAL_S, "o": EVAL_O, "s+o": EVAL_SPO, "s,o": EVAL_S_O}


class EmgError(RuntimeError):
    """A libemgraph_hip call returned a non-zero code."""


_p = C.c_void_p
_i32, _i64, _u64, _f32 = C.c_int32, C.c_int64, C.c_uint64, C.c_float
_int = C.c_int

# name -> (restype, argtypes); every symbol include/emgraph_hip.h declares
SIGNATURES = {
    "emg_version": (_int, []),
    "emg_last_error": (C.c_char_p, []),
    "emg_target": (C.c_char_p, []),
    "emg_source_hash": (C.c_char_p, []),
    "emg_cache_policy_launches": (_i64, []),
    "emg_score_triples": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _i32, _p, _p]),
    "emg_finalize_scores": (_int, [_int, _f32, _p, _i64, _p]),
    "emg_corrupt_codes": (_int, [_i64, _i32, _int, _i64, _p, _u64, _u64, _p, _p, _p, _p]),
    "emg_corrupt_expand": (_int, [_p, _i64, _i32, _p, _p, _p]),
    "emg_train_forward": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _i32, _p, _i32, _p, _p, _p]),
    "emg_loss": (_int, [_int, _p, _p, _i64, _i32, _i32, _f32, _f32, _p, _p, _p, _p]),
    "emg_train_backward": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _i32, _p, _p, _p,
                                  _p, _p, _i64, _p, _p, _p]),
    "emg_apply_workspace_bytes": (_i64, [_i64, _i64]),
    "emg_apply_workspace_bytes_ex": (_i64, [_i64, _i64, _i32]),
    "emg_apply_rows": (_int, [_int, _p, _i64, _i64, _i32, _p, _p, _p, _i32, _p, _i64, _p, _i64,
                              C.POINTER(_f32), _p, _i64, _p]),
    "emg_lp_regularizer": (_int, [_p, _i64, _i64, _i32, _f32, _i32, _f32, _p, _p]),
    "emg_lp_grad_rows": (_int, [_p, _i64, _i64, _i32, _f32, _i32, _p, _i64, _p, _p, _p]),
    "emg_clip_rows": (_int, [_p, _i64, _i64, _i32, _f32, _p]),
    "emg_scatter_rows": (_int, [_p, _i64, _i64, _i32, _p, _i64, _p, _i64, _p]),
    "emg_eval_build_queries": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _int, _p, _i64,
                                      _p, _p]),
    "emg_eval_count": (_int, [_int, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _i32, _f32, _int, _p, _i64, _p, _p, _p]),
    "emg_eval_filter_count": (_int, [_int, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i32, _f32, _int, _p, _p,
                                     _p, _p, _p]),
    "emg_eval_scores_dense": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _p, _i32, _f32, _int, _p, _i64, _p,
                                     _i64, _p]),
    "emg_eval_topn_ws_bytes": (_i64, [_i64, _i64, _i32, _i64]),
    "emg_eval_topn": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i32, _f32, _i32, _p, _p, _i64, _p, _i64,
                             _p, _p, _p]),
    "emg_eval_grid_ws_bytes": (_i64, [_i64, _i32]),
    "emg_eval_grid_count": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i32, _p, _p, _p, _i64, _p, _p, _p]),
    "emg_to_bf16": (_int, [_p, _i64, _i64, _i32, _p, _i64, _p]),
    "emg_to_f16": (_int, [_p, _i64, _i64, _i32, _p, _i64, _p]),
}

class BackwardArgs(C.Structure):
    """mirror of `emg_backward_args` (include/emgraph_hip.h)"""
    _fields_ = [
        ("model", _i32), ("k_int", _i32), ("scale", _f32), ("eta", _i32),
        ("ent", _p), ("n_ent", _i64), ("ld_ent", _i64),
        ("rel", _p), ("n_rel", _i64), ("ld_rel", _i64),
        ("pos", _p), ("B", _i64), ("codes", _p),
        ("fused_loss", _i32), ("margin", _f32), ("loss_accum", _p),
        ("g_pos", _p), ("g_neg", _p),
        ("bw_scores_pos", _p), ("bw_scores_neg", _p),
        ("scores_pos_out", _p), ("scores_neg_out", _p),
        ("contrib_ent", _p), ("contrib_rel", _p), ("ldc", _i64),
        ("single_ent", _p), ("opt", _i32), ("step", _i32), ("hyper", _f32 * 8),
        ("ent_state0", _p), ("ent_state1", _p), ("tag_ent", _p),
        ("fac_ws_ent", _p), ("fac_ws_ent_bytes", _i64),
        ("layout_B", _i64), ("ctl", _p),
        ("lp_accum", _p),
        ("lr_hist", _p),
        ("inplace_window", _i32), ("loss_slots", _i32),
        ("link", _i32), ("sw", _f32), ("edge_w", _p),
    ]


SIGNATURES.update({
    "emg_build_dest": (_int, [_p, _i64, _i32, _p, _p, _p, _p]),
    "emg_train_backward_ex": (_int, [C.POINTER(BackwardArgs), _p]),
    "emg_train_backward_form": (_int, [C.POINTER(BackwardArgs), _i32, C.POINTER(_i32)]),
    "emg_link_scores": (_int, [_i32, _p, _f32, _p, _p, _i64, _i32, _p, _p, _p]),
    "emg_link_grads": (_int, [_p, _p, _p, _p, _i64, _i32, _p]),
    "emg_group_dest": (_int, [_p, _i64, _i64, _p, _i64, _p, _p]),
    "emg_group_dest_keyed": (_int, [_p, _p, _i64, _i64, _p, _i64, _p]),
    "emg_apply_grouped": (_int, [_int, _p, _i64, _i64, _i32, _p, _p, _p, _i32, _p, _i64, _i64, _i32,
                                 C.POINTER(_f32), _p, _p, _i64, _p]),
    "emg_apply_grouped_factored": (_int, [_int, _p, _i64, _i64, _i32, _p, _p, _p, _i32, _p, _i64, _i64, _i32,
                                          C.POINTER(_f32), _p, _p, _i64, _p]),
})

class PrepareArgs(C.Structure):
    """mirror of `emg_prepare_args` (include/emgraph_hip.h)"""
    _fields_ = [
        ("pos", _p), ("B", _i64), ("eta", _i32), ("n_sides", _i32), ("sides", _i32 * 4),
        ("n_choices", _i64), ("entities_list", _p), ("seed", _u64), ("draw_counter0", _u64),
        ("inj_mask", _p), ("inj_repl", _p),
        ("codes", _p),
        ("dest_ent", _p), ("n_extra_ent", _i64), ("n_ent", _i64),
        ("dest_rel", _p), ("n_extra_rel", _i64), ("n_rel", _i64),
        ("ws_ent", _p), ("ws_ent_bytes", _i64), ("ws_rel", _p), ("ws_rel_bytes", _i64),
        ("single_flags", _p),
        ("B_global", _i64), ("row_offset", _i64),
        ("factored", _i32), ("ws_clean", _i32),
        ("layout_B", _i64), ("ctl", _p),
    ]


SIGNATURES.update({"emg_prepare_batch": (_int, [C.POINTER(PrepareArgs), _p])})


class Sampler(C.Structure):
    """mirror of `emg_sampler` (include/emgraph_hip.h): the negative sampler a run binds"""
    _fields_ = [
        ("size", _i64),
        ("keep_thr", _p),
        ("known_keys", _p), ("n_known", _i64),
        ("n_ent", _i64), ("n_rel", _i64),
        ("retries", _i32), ("reserved0", _i32),
        ("stats", _p),
        ("pool_ptr", _p), ("pool_idx", _p),     # typed negatives: grown at the end (SAMPLER_SIZE_V1: the first layout)
    ]


SAMPLER_SIZE_V1 = Sampler.pool_ptr.offset   # sizeof(emg_sampler) before the pools: still accepted by emg_sampler_bind

SIGNATURES.update({
    "emg_sampler_bind": (_int, [C.POINTER(Sampler)]),
    "emg_sampler_bound": (_int, []),
    "emg_corrupt_codes_sampled": (_int, [_p, _i64, _i32, _int, _i64, _p, _u64, _u64, _p, _p, _p, _p]),
})

SIGNATURES.update({
    "emg_eval_pos_int_bf16": (_int, [_int, _p, _i64, _i32, _f32, _p, _i64, _int, _p, _i64, _p, _p, _p]),
    "emg_eval_count_bf16": (_int, [_int, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _p, _i64, _i32, _f32, _p, _p, _i32, _p]),
    "emg_eval_filter_count_bf16": (_int, [_int, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i32, _f32, _p, _p,
                                          _p, _p, _p]),
    "emg_eval_scores_dense_bf16": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _p, _i32, _f32, _p, _i64, _p]),
    "emg_eval_prefilter_bounds": (_int, [_p, _i64, _i64, _p, _i64, _i32, _p, _p]),
    "emg_eval_prefilter_band": (_int, [_p, _i64, _i64, _p, _i64, _i32, _p, _p, _p]),
    "emg_eval_prefilter_f16": (_int, [_int, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i32, _f32, _p, _p, _p, _i64, _p]),
    "emg_eval_prefilter_f16_ties": (_int, [_int, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i32, _f32, _p, _p, _p, _p, _i64, _p]),
    "emg_eval_prefilter_segments": (_i64, [_i64, _i64]),
    "emg_eval_prefilter_segments_k": (_i64, [_i64, _i64, _i32]),
    "emg_eval_prefilter_waves": (_i32, [_i32]),
    "emg_eval_prefilter_max_cols": (_i32, []),
    "emg_eval_rescore_pairs_rows": (_int, [_int, _p, _i64, _p, _p, _i64, _i64, _i32, _f32, _p, _i64, _p, _i64, _i32, _i32, _p, _p, _p]),
    "emg_eval_prefilter_ld": (_i64, [_i32]),
    "emg_eval_rescore_tiles_ws_bytes": (_i64, [_i64]),
    "emg_eval_rescore_pairs_tiles": (_int, [_int, _p, _i64, _p, _p, _i64, _i64, _i64, _i32, _f32, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _p, _p]),
    "emg_eval_rescore_pairs": (_int, [_int, _p, _i64, _p, _p, _i64, _i64, _i32, _f32, _p, _i64, _p, _i64, _p, _p, _p]),
    "emg_eval_rescore_pairs_ex": (_int, [_int, _p, _i64, _p, _p, _i64, _i64, _i32, _f32, _p, _i64, _p, _i64, _i32, _p, _p, _p]),
    "emg_to_f16_l2": (_int, [_p, _i64, _i64, _i32, _int, _p, _i64, _p, _p, _p]),
    "emg_eval_l2_thresholds": (_int, [_p, _i64, _i64, _p, _p, _p, _i32, _p, _p]),
    "emg_eval_prefilter_f16_thr": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i32, _p, _p, _p, _i64, _p]),
    "emg_eval_sad_range": (_int, [_p, _i64, _i64, _p, _i64, _i64, _i32, _p, _p]),
    "emg_eval_sad_ld": (_i64, [_i32]),
    "emg_eval_sad_quantize": (_int, [_p, _i64, _i64, _i32, _p, _p, _i64, _p]),
    "emg_eval_sad_thresholds": (_int, [_p, _i64, _i32, _p, _p, _p, _p]),
    "emg_eval_sad_segments": (_i64, [_i64, _i64]),
    "emg_eval_prefilter_sad": (_int, [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i32, _p, _p, _p, _i64, _p]),
})

# ranking through the score link (additions at ABI 9)
SIGNATURES.update({
    "emg_eval_build_queries_link": (_int, [_int, _i32, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _int, _p, _i64, _p, _p]),
    "emg_eval_count_link": (_int, [_int, _i32, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _i32, _f32, _int, _p, _p, _p]),
    "emg_eval_filter_count_link": (_int, [_int, _i32, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i32, _f32, _int, _p, _p, _p, _p, _p]),
    "emg_eval_rescore_pairs_link": (_int, [_int, _i32, _p, _i64, _p, _p, _i64, _i64, _i32, _f32, _p, _i64, _p, _i64, _i32, _i32, _p, _p, _p]),
    "emg_eval_link_order_w": (_i32, [_i32]),
    "emg_eval_link_order_violations": (_int, [_i32, _i32, C.c_uint32, C.c_uint32, _p, _p]),
    "emg_eval_link_thresholds": (_int, [_i32, _p, _p, _i64, _f32, _p, _p, _p, _p]),
    "emg_eval_prefilter_f16_thr4": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i32, _p, _p, _p, _p, _i64, _p]),
})

class StepArgs(C.Structure):
    """mirror of `emg_step_args` (include/emgraph_hip.h)"""
    _fields_ = [
        ("model", _i32), ("k_int", _i32), ("scale", _f32), ("eta", _i32), ("n_sides", _i32), ("sides", _i32 * 4),
        ("ent", _p), ("n_ent", _i64), ("ld_ent", _i64), ("rel", _p), ("n_rel", _i64), ("ld_rel", _i64),
        ("ent_state0", _p), ("ent_state1", _p), ("rel_state0", _p), ("rel_state1", _p),
        ("tag_ent", _p), ("tag_rel", _p),
        ("opt", _i32), ("step", _i32), ("hyper", _f32 * 8),
        ("pos", _p), ("B", _i64),
        ("n_choices", _i64), ("entities_list", _p), ("seed", _u64), ("draw_counter0", _u64),
        ("inj_mask", _p), ("inj_repl", _p),
        ("loss", _i32), ("margin", _f32), ("alpha", _f32), ("loss_accum", _p),
        ("inplace", _i32),
        ("workspace", _p), ("workspace_bytes", _i64),
        ("link", _i32), ("sw", _f32), ("edge_w", _p),
    ]


SIGNATURES.update({
    "emg_corrupt_fit": (_int, [_p, _i64, _i32, _int, _i64, _p, _i64, _u64, _u64, _p, _p]),
    "emg_rank_1vsall": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _int, _p, _i64, _p, _p, _int,
                               _int, _p, _p]),
    "emg_train_step_workspace_bytes": (_i64, [_i64, _i32, _i32, _i64, _i64]),
    "emg_train_step": (_int, [C.POINTER(StepArgs), _p]),
})

class ApplyArgs(C.Structure):
    """mirror of `emg_apply_args`"""
    _fields_ = [
        ("opt", _i32), ("k_int", _i32), ("table", _p), ("n_rows", _i64), ("ld", _i64),
        ("state0", _p), ("state1", _p), ("tag", _p), ("step", _i32), ("skip_single", _i32),
        ("contrib", _p), ("ldc", _i64), ("n_contrib", _i64),
        ("hyper", _f32 * 8), ("lp_accum", _p), ("workspace", _p), ("workspace_bytes", _i64),
        ("factored", _i32), ("table_index", _i32),
        ("layout_n", _i64), ("ctl", _p),
        ("deferred_dense", _i32), ("reserved1", _i32),
    ]


SIGNATURES.update({
    "emg_apply_grouped_ex": (_int, [C.POINTER(ApplyArgs), _p]),
    "emg_apply_grouped_pair": (_int, [C.POINTER(ApplyArgs), C.POINTER(ApplyArgs), _p]),
    "emg_deferred_catchup": (_int, [_int, _p, _i64, _i64, _i32, _p, _p, _p, C.POINTER(_f32), _p, _i32, _p, _p, _i64, _i64, _i32, _i64, _p]),
    "emg_deferred_materialize": (_int, [_int, _p, _i64, _i64, _i32, _p, _p, _p, C.POINTER(_f32), _p, _i32, _p, _p]),
})


class PlanSlot(C.Structure):
    """mirror of `emg_plan_slot`"""
    _fields_ = [("codes", _p), ("dest_ent", _p), ("dest_rel", _p), ("single", _p),
                ("ws_ent", _p), ("ws_ent_bytes", _i64), ("ws_rel", _p), ("ws_rel_bytes", _i64)]


class PlanConfig(C.Structure):
    """mirror of `emg_plan_config`"""
    _fields_ = [
        ("model", _i32), ("k_int", _i32), ("scale", _f32), ("eta", _i32), ("n_sides", _i32), ("sides", _i32 * 4),
        ("ent", _p), ("n_ent", _i64), ("ld_ent", _i64), ("rel", _p), ("n_rel", _i64), ("ld_rel", _i64),
        ("ent_state0", _p), ("ent_state1", _p), ("rel_state0", _p), ("rel_state1", _p), ("tag_ent", _p), ("tag_rel", _p),
        ("opt", _i32), ("loss", _i32), ("margin", _f32), ("alpha", _f32),
        ("seed", _u64), ("batches_count", _i64),
        ("X", _p), ("n_triples", _i64),
        ("cap_B", _i64),
        ("scores", _p), ("g", _p), ("contrib_ent", _p), ("contrib_rel", _p), ("ldc", _i64),
        ("loss_accum", _p), ("lp_sum", _p),
        ("factored", _i32), ("loss_slots", _i32),
        ("lp_lambda_ent", _f32), ("lp_lambda_rel", _f32), ("lp_p", _i32),
        ("fused", _i32), ("inplace", _i32), ("normalize", _i32),
        ("n_slots", _i32), ("slots", PlanSlot * 4),
        ("aux_min_rows", _i64),
        ("ctl_buf", _p), ("ctl_bytes", _i64),
        ("lr_t_hist", _p),
        ("link", _i32), ("reserved2", _i32), ("edge_w", _p), ("link_fac", _p),
    ]


class PlanBatch(C.Structure):
    """mirror of `emg_plan_batch`"""
    _fields_ = [("start", _i64), ("B", _i64), ("epoch", _i32), ("batch", _i32),
                ("n_choices", _i64), ("entities_list", _p), ("inj_mask", _p), ("inj_repl", _p),
                ("sw", _f32), ("reserved0", _i32)]


SIGNATURES.update({
    "emg_plan_create": (_int, [C.POINTER(PlanConfig), C.POINTER(_p)]),
    "emg_plan_step": (_int, [_p, C.POINTER(PlanBatch), _i32, C.POINTER(_f32), C.POINTER(PlanBatch), _i32, _p]),
    "emg_plan_graph_ok": (_int, [_p]),
    "emg_plan_deferred_ok": (_int, [_i64, _i32, _i64, _i64]),
    "emg_plan_run": (_int, [_p, C.POINTER(PlanBatch), _i32, _i32, C.POINTER(_f32), _p]),
    "emg_plan_timing": (_int, [_p, _i32]),
    "emg_plan_stage_ms": (_int, [_p, C.POINTER(_f32), C.POINTER(_i32)]),
    "emg_plan_destroy": (_int, [_p]),
    "emg_init_table": (_int, [_int, _p, _i64, _i64, _i32, _f32, _f32, _u64, _u64, _p]),
})

class CalibArgs(C.Structure):
    """mirror of `emg_calib_args` (include/emgraph_hip.h)"""
    _fields_ = [
        ("model", _i32), ("k_int", _i32), ("scale", _f32), ("reserved0", _i32),
        ("ent", _p), ("n_ent", _i64), ("ld_ent", _i64), ("rel", _p), ("n_rel", _i64), ("ld_rel", _i64),
        ("pos", _p), ("B", _i64),
        ("scores_pos", _p),
        ("seed", _u64), ("draw_counter", _u64),
        ("label_pos", C.c_double), ("label_neg", C.c_double),
        ("weight_pos", C.c_double), ("weight_neg", C.c_double),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("state", _p),
        ("workspace", _p), ("workspace_bytes", _i64),
        ("dbg_neg", _p), ("dbg_scores", _p),
    ]


_f64 = C.c_double
SIGNATURES.update({
    "emg_calib_ws_bytes": (_i64, [_i64]),
    "emg_calib_step": (_int, [C.POINTER(CalibArgs), _p]),
    "emg_calib_moments": (_int, [_p, _i64, _p, _i64, _f64, _f64, _f64, _f64, _f64, _f64, _p, _p, _i64, _p]),
    "emg_calib_proba": (_int, [_p, _i64, _f32, _f32, _p, _p]),
})

# relation prediction (csrc/emg_relrank.hip; additions at ABI 9)
SIGNATURES.update({
    "emg_eval_rel_rotate_image": (_int, [_p, _i64, _i64, _i32, _p, _i64, _p]),
    "emg_eval_rel_count": (_int, [_int, _i32, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _p, _p, _i64, _p, _p,
                                  _p, _p, _p, _p, _p]),
    "emg_eval_rel_scores_dense": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _p, _i64, _p, _i64, _p]),
    "emg_eval_rel_topn": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _i32, _p, _p, _p]),
})

# RotatE exact-fast ranking (csrc/emg_rank_rotate.hip; additions at ABI 9)
ENOSUP = -3   # EMG_ENOSUP
SIGNATURES.update({
    "emg_eval_rotate_ld": (_i64, [_i32]),
    "emg_eval_rotate_image": (_int, [_p, _i64, _i64, _i32, _f32, _p, _i64, _p, _p, _i32, _p]),
    "emg_eval_rotate_thresholds": (_int, [_p, _p, _i64, _i32, _f32, _p, _p, _p, _p, _p]),
    "emg_eval_prefilter_rotate_segments": (_i64, [_i64, _i64]),
    "emg_eval_prefilter_rotate": (_int, [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i32, _p, _p, _p, _i64, _p]),
    "emg_eval_prefilter_rotate_dense": (_int, [_p, _i64, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _p]),
})

# typed ranking (csrc/emg_rank_typed.hip; an addition at ABI 9)
SIGNATURES.update({
    "emg_eval_count_grouped": (_int, [_int, _p, _i64, _p, _i64, _p, _p, _i64, _i64, _p, _p, _i64, _i32, _f32, _p, _p, _p]),
})

# sampled ranking (csrc/emg_rank_lists.hip; additions at ABI 9)
SIGNATURES.update({
    "emg_eval_count_lists": (_int, [_int, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _i64, _i32, _p, _p, _i32, _f32, _p, _p, _p]),
    "emg_eval_draw_candidates": (_int, [_i64, _i64, _int, _i32, _i64, C.c_uint64, _p, _i64, _p]),
})


class SharedArgs(C.Structure):
    """mirror of `emg_shared_args` (include/emgraph_hip.h): shared negatives"""
    _fields_ = [
        ("model", _i32), ("k_int", _i32), ("scale", _f32), ("eta_total", _i32),
        ("ent", _p), ("n_ent", _i64), ("ld_ent", _i64),
        ("rel", _p), ("n_rel", _i64), ("ld_rel", _i64),
        ("pos", _p), ("B", _i64), ("C", _i32), ("reserved0", _i32),
        ("chunk_codes", _p),
        ("scores_pos", _p), ("scores_neg", _p),
        ("g_pos", _p), ("g_neg", _p),
        ("raw_pos", _p), ("raw_neg", _p),
        ("contrib_ent", _p), ("contrib_rel", _p), ("ldc", _i64),
        ("dest_ent", _p), ("dest_rel", _p),
    ]


SHARED_NEGATIVES_MAX = 256   # chunk sizes emg_shared_forward / emg_shared_backward take

# shared negatives (csrc/emg_shared.hip; additions at ABI 9)
SIGNATURES.update({
    "emg_shared_forward": (_int, [C.POINTER(SharedArgs), _p]),
    "emg_shared_backward": (_int, [C.POINTER(SharedArgs), _p]),
})

class RelnegArgs(C.Structure):
    """mirror of `emg_relneg_args` (include/emgraph_hip.h): relation negatives"""
    _fields_ = [
        ("model", _i32), ("k_int", _i32), ("scale", _f32), ("eta", _i32),
        ("ent", _p), ("n_ent", _i64), ("ld_ent", _i64),
        ("rel", _p), ("n_rel", _i64), ("ld_rel", _i64),
        ("pos", _p), ("B", _i64),
        ("codes", _p),
        ("scores_pos", _p), ("scores_neg", _p),
        ("g_pos", _p), ("g_neg", _p),
        ("raw_pos", _p), ("raw_neg", _p),
        ("contrib_ent", _p), ("contrib_rel", _p), ("ldc", _i64),
        ("dest_ent", _p), ("dest_rel", _p),
    ]


# relation negatives (csrc/emg_relneg.hip; additions at ABI 9).  SIDE_P is the host's name of the third corruption side: the
# library's sampler is asked for it as a forced side over n_rel - 1 choices (the keep_subject bit of its codes stays zero)
SIDE_P = 3
SIDE_IDS["p"] = SIDE_P
SIGNATURES.update({
    "emg_relneg_forward": (_int, [C.POINTER(RelnegArgs), _p]),
    "emg_relneg_backward": (_int, [C.POINTER(RelnegArgs), _p]),
})

class BatchregArgs(C.Structure):
    """mirror of `emg_batchreg_args` (include/emgraph_hip.h): the batch-local Lp / N3 regulariser"""
    _fields_ = [
        ("k_int", _i32), ("p", _i32),
        ("form_ent", _i32), ("form_rel", _i32),
        ("coef_g_ent", _f32), ("coef_v_ent", _f32),
        ("coef_g_rel", _f32), ("coef_v_rel", _f32),
        ("ent", _p), ("n_ent", _i64), ("ld_ent", _i64),
        ("rel", _p), ("n_rel", _i64), ("ld_rel", _i64),
        ("pos", _p), ("B", _i64),
        ("contrib_ent", _p), ("contrib_rel", _p), ("ldc", _i64),
        ("dest_ent", _p), ("dest_rel", _p),
        ("value", _p),
    ]


# batch-local regulariser (csrc/emg_batchreg.hip; an addition at ABI 9)
BATCHREG_PLAIN, BATCHREG_MODULUS = range(2)   # EMG_BATCHREG_*
SIGNATURES.update({
    "emg_batchreg": (_int, [C.POINTER(BatchregArgs), _p]),
})

METRIC_L2, METRIC_COSINE = range(2)   # EMG_METRIC_*
SIGNATURES.update({
    "emg_rows_normalize": (_int, [_p, _i64, _i64, _i32, _p, _i64, _p]),
    "emg_rows_within": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i32, _i64, _f32, _p, _p, _p, _p, _i64, _p, _p]),
    "emg_rows_dbscan_ws_bytes": (C.c_size_t, [_i64, _i32]),
    "emg_rows_dbscan": (_int, [_int, _p, _i64, _i64, _i32, _f32, _i32, _p, _p, _p, _p, C.c_size_t, _p]),
    "emg_rows_kmeans_ws_bytes": (C.c_size_t, [_i64, _i64, _i32]),
    "emg_rows_kmeans": (_int, [_p, _i64, _i64, _i32, _p, _i64, _i64, _i32, _f64, _p, _p, _p, C.c_size_t, _p]),
    "emg_rows_kmeans_seed": (_int, [_p, _i64, _i64, _i32, _i64, _i64, C.POINTER(_f64), _p, _i64, _p, _p, C.c_size_t, _p]),
})

_lib = None


def load():
    """Load (once) and return the ctypes handle.  Raises if the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EmgError(
            "libemgraph_hip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or emgraph_amd/csrc/build.sh.  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    ver = lib.emg_version()
    if ver != ABI_VERSION:
        raise EmgError("libemgraph_hip ABI version %d != expected %d" % (ver, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().emg_last_error().decode("utf-8", "replace")
        raise EmgError("%s failed (code %d): %s" % (what or "libemgraph_hip call", rc, msg))
