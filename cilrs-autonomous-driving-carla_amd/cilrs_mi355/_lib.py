"""ctypes binding of libcilrs_hip.so (C-ABI declared in include/cilrs_hip.h).

The library is the product: there is NO CPU or eager-PyTorch fallback.  If the shared object is
missing or a call fails, a RuntimeError is raised with the library's own message.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CILRS_LIB: another build of the same library (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("CILRS_LIB") or os.path.join(_HERE, "libcilrs_hip.so")

c_float_p = C.POINTER(C.c_float)
vp = C.c_void_p
sz = C.c_size_t
i32 = C.c_int
i64 = C.c_int64
f32 = C.c_float
f64 = C.c_double
u64 = C.c_uint64


class Buffers(C.Structure):
    """struct cilrs_buffers"""
    _fields_ = [("params", vp), ("grads", vp), ("bn_running", vp), ("bn_nbt", vp),
                ("workspace", vp)]


class AdamArgs(C.Structure):
    """struct cilrs_adam_args"""
    _fields_ = [("exp_avg", vp), ("exp_avg_sq", vp), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("step", C.c_int64), ("grad_scale", C.c_float)]


class ReplayConfig(C.Structure):
    """struct cilrs_replay_config"""
    _fields_ = [(k, C.c_double) for k in (
        "dt_s", "speed_unit_ms", "wheelbase_m", "max_wheel_rad", "lookahead_s", "min_lookahead_m",
        "fx", "fy", "cx", "cy", "height_m", "max_lateral_m", "max_yaw_rad", "recover_m")] \
        + [("taps", C.c_double * 8), ("ntaps", C.c_int), ("closed_loop", C.c_int)]


# symbol -> (restype, argtypes); every symbol include/cilrs_hip.h declares is listed here
SIGNATURES = {
    "cilrs_version": (i32, []),
    "cilrs_last_error": (C.c_char_p, []),
    "cilrs_num_params": (i32, []),
    "cilrs_num_bn": (i32, []),
    "cilrs_param_arena_floats": (sz, []),
    "cilrs_param_count": (sz, []),
    "cilrs_param_info": (i32, [i32, C.c_char_p, i32, C.POINTER(sz), C.POINTER(sz),
                               C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_bn_info": (i32, [i32, C.c_char_p, i32, C.POINTER(i32), C.POINTER(sz), C.POINTER(sz)]),
    "cilrs_bn_arena_floats": (sz, []),
    "cilrs_num_variants": (i32, []),
    "cilrs_variant_num_params": (i32, [i32]),
    "cilrs_variant_num_bn": (i32, [i32]),
    "cilrs_variant_param_arena_floats": (sz, [i32]),
    "cilrs_variant_param_count": (sz, [i32]),
    "cilrs_variant_bn_arena_floats": (sz, [i32]),
    "cilrs_variant_feature_width": (i32, [i32]),
    "cilrs_variant_param_info": (i32, [i32, i32, C.c_char_p, i32, C.POINTER(sz), C.POINTER(sz),
                                       C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_variant_bn_info": (i32, [i32, i32, C.c_char_p, i32, C.POINTER(i32), C.POINTER(sz),
                                    C.POINTER(sz)]),
    "cilrs_net_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
    "cilrs_net_create_variant": (i32, [i32, i32, i32, i32, C.POINTER(vp)]),
    "cilrs_net_create_ex": (i32, [i32, i32, i32, i32, C.c_uint, C.POINTER(vp)]),
    "cilrs_net_destroy": (None, [vp]),
    "cilrs_net_workspace_bytes": (sz, [vp]),
    "cilrs_net_status_offset": (sz, [vp]),
    "cilrs_net_set_weights_key": (i32, [vp, u64]),
    "cilrs_net_activation_info": (i32, [vp, i32, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz),
                                        C.POINTER(i32)]),
    "cilrs_net_pool_argmax_info": (i32, [vp, C.POINTER(sz), C.POINTER(sz)]),
    "cilrs_net_head_activation_info": (i32, [vp, i32, i32, C.POINTER(sz), C.POINTER(i32),
                                             C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_dropout": (i32, [vp, i32, i32, i32, f32, u64, i32, vp]),
    "cilrs_heads_mc_scratch_floats": (sz, [i32, i32, i32]),
    "cilrs_heads_mc": (i32, [i32, vp, vp, i32, vp, vp, i32, i32, f32, u64, vp, vp, vp, vp, sz, vp, vp]),
    "cilrs_net_heads_mc": (i32, [vp, C.POINTER(Buffers), vp, vp, i32, f32, u64, vp, vp, vp, vp, sz,
                                 vp]),
    "cilrs_heads_input_grad": (i32, [i32, vp, vp, i32, vp, i32, vp, vp, c_float_p, i32, vp, vp, vp, vp]),
    "cilrs_gradcam_map": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "cilrs_gradcam_scratch_floats": (sz, [i32, i32]),
    "cilrs_net_gradcam_info": (i32, [vp, i32, C.POINTER(sz), C.POINTER(sz), C.POINTER(i32),
                                     C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_net_gradcam": (i32, [vp, C.POINTER(Buffers), vp, vp, c_float_p, i32, vp, vp, vp, vp, vp, sz,
                                vp]),
    "cilrs_feature_moments_doubles": (sz, [i32, i32]),
    "cilrs_feature_moments": (i32, [vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]),
    "cilrs_feature_novelty_scratch_floats": (sz, [i32, i32]),
    "cilrs_feature_novelty": (i32, [vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp, vp]),
    "cilrs_net_feature_moments": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp]),
    "cilrs_net_novelty": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, sz, vp]),
    "cilrs_kcenter_scratch_bytes": (sz, [i32]),
    "cilrs_kcenter_cover": (i32, [vp, C.c_long, i32, i32, vp, C.c_long, i32, vp, vp]),
    "cilrs_kcenter_greedy": (i32, [vp, C.c_long, i32, i32, vp, i32, vp, vp, vp, sz, vp]),
    "cilrs_knn_scratch_bytes": (sz, [i32, i32, i32]),
    "cilrs_knn": (i32, [vp, C.c_long, i32, i32, vp, C.c_long, i32, vp, i32, vp, vp, vp, sz, vp]),
    "cilrs_knn_join_candidates": (i32, [i32]),
    "cilrs_knn_join_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "cilrs_knn_join": (i32, [vp, C.c_long, i32, i32, vp, C.c_long, i32, vp, i32, vp, vp, vp, vp, vp, sz, vp]),
    "cilrs_kmeans_scratch_bytes": (sz, [i32, i32, i32]),
    "cilrs_kmeans_assign": (i32, [vp, C.c_long, i32, i32, vp, C.c_long, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "cilrs_kmeans_update": (i32, [vp, C.c_long, i32, i32, vp, vp, C.c_long, i32, vp, vp, sz, vp]),
    "cilrs_kmeans_lloyd": (i32, [vp, C.c_long, i32, i32, vp, C.c_long, i32, i32, vp, vp, vp, vp, vp, vp, sz,
                                 vp]),
    "cilrs_feature_whiten_scratch_floats": (sz, [i32, i32]),
    "cilrs_feature_whiten": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "cilrs_net_knn_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "cilrs_net_knn": (i32, [vp, C.POINTER(Buffers), vp, C.c_long, i32, vp, vp, i32, vp, vp, vp, sz, vp]),
    "cilrs_net_infer16_conv_info": (i32, [vp, i32, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz),
                                          C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_net_infer16_io_info": (i32, [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz),
                                        C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_net_forward": (i32, [vp, C.POINTER(Buffers), vp, C.c_long, C.c_long, C.c_long,
                                C.c_long, vp, vp, i32, f32, u64, vp, vp, vp]),
    "cilrs_net_forward_frozen": (i32, [vp, C.POINTER(Buffers), vp, C.c_long, C.c_long, C.c_long,
                                       C.c_long, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_u8": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_camera": (i32, [vp, C.POINTER(Buffers), vp, i32, i32, i32, C.c_long,
                                       C.c_long, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_frozen_u8": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_frozen_camera": (i32, [vp, C.POINTER(Buffers), vp, i32, i32, i32, C.c_long,
                                              C.c_long, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_u8_f16": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_u8_f16_graph": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_u8_graph": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_u8_b1": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_camera_b1": (i32, [vp, C.POINTER(Buffers), vp, i32, i32, i32, C.c_long, vp, vp,
                                          vp, vp, i32, vp]),
    "cilrs_net_forward_u8_b1_post": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp, i32, vp]),
    "cilrs_net_forward_u8_b1_sync": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_b1_stages": (i32, [vp]),
    "cilrs_net_b1_stage_info": (i32, [vp, i32] + [C.POINTER(i32)] * 8),
    "cilrs_net_b1_set_epoch": (i32, [vp, C.POINTER(Buffers), i32, vp]),
    "cilrs_net_wino_convs": (i32, [vp]),
    "cilrs_net_forward_ft": (i32, [vp, C.POINTER(Buffers), vp, C.c_long, C.c_long, C.c_long,
                                   C.c_long, vp, vp, i32, i32, u64, f32, u64, vp, vp, vp]),
    "cilrs_net_ft_wino_convs": (i32, [vp]),
    "cilrs_net_ft_cut": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_net_b1_stage_us": (i32, [vp, C.POINTER(Buffers), c_float_p, c_float_p, i32]),
    "cilrs_net_forward_u8_bf16": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_net_forward_u8_bf16_graph": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp, vp, vp]),
    "cilrs_loss_fwd_bwd": (i32, [vp, vp, vp, vp, i32, i32, c_float_p, f32, vp, vp, vp, vp]),
    "cilrs_net_backward": (i32, [vp, C.POINTER(Buffers), vp, vp, i32, i32, vp]),
    "cilrs_net_backward_data": (i32, [vp, C.POINTER(Buffers), vp, vp, i32, i32, vp]),
    "cilrs_net_input_grads": (i32, [vp, C.POINTER(Buffers), vp, C.c_long, C.c_long, C.c_long,
                                    C.c_long, vp, vp]),
    "cilrs_stem_conv_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "cilrs_stem_conv_wgrad_scratch_floats": (sz, [i32, i32, i32]),
    "cilrs_stem_conv_wgrad": (i32, [vp, vp, vp, vp, sz, i32, i32, i32, vp]),
    "cilrs_stem_conv_dgrad": (i32, [vp, vp, vp, C.c_long, C.c_long, C.c_long, C.c_long, i32, i32,
                                    i32, vp]),
    "cilrs_net_backward_step": (i32, [vp, C.POINTER(Buffers), vp, vp, vp, vp]),
    "cilrs_segment_range": (i32, [i32, C.POINTER(sz), C.POINTER(sz)]),
    "cilrs_variant_segment_range": (i32, [i32, i32, C.POINTER(sz), C.POINTER(sz)]),
    "cilrs_sqnorm_scratch_bytes": (sz, []),
    "cilrs_grad_sqnorm": (i32, [vp, sz, f32, vp, vp, vp]),
    "cilrs_adam_step": (i32, [vp, vp, vp, vp, sz, f64, f64, f64, f64, f64, i64, vp, f32, vp]),
    "cilrs_adam_step_groups": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, vp, f64, f64, f64, f64, vp, f32,
                                     vp]),
    "cilrs_scale": (i32, [vp, sz, vp, f32, vp]),
    "cilrs_ema_update": (i32, [vp, vp, sz, f32, vp]),
    "cilrs_adam_step_ema": (i32, [vp, vp, vp, vp, sz, f64, f64, f64, f64, f64, i64, vp, f32, vp, f32,
                                  vp]),
    "cilrs_adam_step_groups_ema": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, vp, f64, f64, f64, f64, vp,
                                         f32, vp, f32, vp]),
    "cilrs_swap": (i32, [vp, vp, sz, vp]),
    "cilrs_optim_chunk_floats": (i32, []),
    "cilrs_optim_table_bytes": (sz, [vp, i32]),
    "cilrs_optim_table_create": (i32, [vp, vp, i32, sz, vp, sz, vp, C.POINTER(vp)]),
    "cilrs_optim_table_destroy": (None, [vp]),
    "cilrs_optim_scratch_bytes": (sz, [vp]),
    "cilrs_optim_step": (i32, [i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, f64, f64, f64,
                               f64, f64, vp, f32, vp, vp, vp]),
    "cilrs_sam_chunk_floats": (i32, []),
    "cilrs_sam_scratch_bytes": (sz, [sz]),
    "cilrs_sam_perturb": (i32, [vp, vp, vp, sz, f64, i32, vp, vp, vp]),
    "cilrs_sam_restore": (i32, [vp, vp, sz, vp]),
    "cilrs_loss_fwd_bwd_rows": (i32, [vp, vp, vp, vp, i32, i32, c_float_p, f32, vp, vp, vp, vp, vp,
                                      vp]),
    "cilrs_priority_max_batch": (i32, []),
    "cilrs_priority_fill": (i32, [vp, i64, vp, vp, vp]),
    "cilrs_priority_update": (i32, [vp, i64, vp, vp, vp, f64, f64, vp, i32, vp]),
    "cilrs_priority_scratch_bytes": (sz, [i64]),
    "cilrs_priority_draw": (i32, [vp, i64, vp, i64, u64, u64, i32, i32, f64, vp, vp, vp, vp, vp]),
    "cilrs_augment_u8": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    "cilrs_batch_assemble": (i32, [vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp,
                                   vp]),
    "cilrs_augment_weather_u8": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "cilrs_batch_assemble_weather": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp,
                                           vp, vp, vp]),
    "cilrs_augment_view_u8": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "cilrs_batch_assemble_view": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp,
                                        vp, vp, vp, vp]),
    "cilrs_replay_state_doubles": (i32, []),
    "cilrs_replay_metric_doubles": (i32, []),
    "cilrs_replay_begin": (i32, [C.POINTER(ReplayConfig), i32, i32, i64, vp, vp, vp, vp, vp, vp, vp,
                                 vp, vp]),
    "cilrs_replay_step": (i32, [C.POINTER(ReplayConfig), i32, i32, vp, vp, vp, i64, vp, vp, vp, vp,
                                vp, vp, vp, vp]),
    "cilrs_replay_finish": (i32, [C.POINTER(ReplayConfig), i32, i32, vp, vp, vp, i64, vp, vp, vp, vp,
                                  vp, vp]),
    "cilrs_eval_acc_doubles": (i32, []),
    "cilrs_eval_accumulate": (i32, [vp, vp, vp, vp, vp, i32, vp, vp, vp]),
    "cilrs_net_profile_enable": (i32, [vp, i32]),
    "cilrs_net_profile_collect": (i32, [vp]),
    "cilrs_net_profile_count": (i32, [vp]),
    "cilrs_net_profile_entry": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(C.c_longlong),
                                      C.POINTER(f64), C.POINTER(f64), C.POINTER(f64)]),
    "cilrs_net_profile_reset": (i32, [vp]),
    "cilrs_conv2d_fwd": (i32, [vp, vp, vp] + [i32] * 11 + [vp, sz, vp]),
    "cilrs_conv2d_dgrad": (i32, [vp, vp, vp, vp] + [i32] * 11 + [vp, sz, vp]),
    "cilrs_conv2d_fwd_stats": (i32, [vp, vp, vp, vp, C.POINTER(i32)] + [i32] * 10 + [vp, sz, vp]),
    "cilrs_conv2d_dgrad_bnbwd": (i32, [vp] * 7 + [i32, vp, C.POINTER(i32)] + [i32] * 10
                                 + [vp, sz, vp]),
    "cilrs_conv2d_takes_classes": (i32, [i32] * 9 + [sz, i32]),
    "cilrs_conv2d_plan_info": (i32, [i32] * 9 + [sz, i32, i32] + [C.POINTER(i32)] * 4),
    "cilrs_net_conv_classes": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32)]),
    "cilrs_conv2d_wgrad_scratch_floats": (sz, [i32] * 9),
    "cilrs_conv2d_wgrad": (i32, [vp, vp, vp, vp] + [i32] * 10 + [vp]),
    "cilrs_conv2d_16_scratch_halfs": (sz, [i32] * 8),
    "cilrs_conv2d_fwd_16": (i32, [vp, vp, vp, vp] + [i32] * 9 + [vp, vp]),
    "cilrs_conv2d_dgrad_16": (i32, [vp, vp, vp, vp] + [i32] * 9 + [vp, vp]),
    "cilrs_conv2d_wgrad_16_scratch_floats": (sz, [i32] * 8),
    "cilrs_conv2d_wgrad_16": (i32, [vp, vp, vp, vp] + [i32] * 9 + [vp, vp]),
    "cilrs_conv2d_train_16": (i32, [vp] * 9 + [i32, vp] + [i32] * 12 + [vp, vp]),
    "cilrs_conv2d_infer_16": (i32, [vp] * 5 + [i32] * 11 + [vp]),
    "cilrs_stem_fold_16": (i32, [vp, vp, vp, vp, i32, vp]),
    "cilrs_stem_infer_16": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "cilrs_maxpool_infer_16": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "cilrs_avgpool_infer_16": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "cilrs_bn16_train_fwd": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, i32,
                                   vp, vp, vp, i32, vp]),
    "cilrs_bn16_bwd": (i32, [vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
    "cilrs_conv2d_wino_split": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp]),
    "cilrs_conv2d_wino_scratch_floats": (sz, [i32, i32]),
    "cilrs_conv2d_wino_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "cilrs_conv2d_wino_fold_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32,
                                         vp, vp]),
    "cilrs_wino_filter_transform": (i32, [vp, vp, i32, i32, i32, vp]),
    "cilrs_conv2d_wino_stamps": (i32, [vp]),
    "cilrs_conv2d_wino_pre": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cilrs_conv2d_wino_dgrad": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "cilrs_conv2d_wino_wgrad_scratch_floats": (sz, [i32, i32, i32, i32, i32]),
    "cilrs_conv2d_wino_wgrad": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
    "cilrs_bn_partial_floats": (sz, [i32]),
    "cilrs_variant_bn_stats_doubles": (sz, [i32]),
    "cilrs_variant_bn_stats_info": (i32, [i32, i32, C.POINTER(i32), C.POINTER(sz), C.POINTER(sz)]),
    "cilrs_net_bn_layer_info": (i32, [vp, i32, C.POINTER(sz), C.POINTER(i32), C.POINTER(i32),
                                      C.POINTER(i32)]),
    "cilrs_net_forward_bn_stats": (i32, [vp, C.POINTER(Buffers), vp, C.c_long, C.c_long, C.c_long, C.c_long, vp, vp]),
    "cilrs_bn_stats_finalize": (i32, [i32, vp, i32, vp, vp, vp]),
    "cilrs_bn_train_stats": (i32, [vp, i32, i32, vp, vp, vp]),
    "cilrs_bn_train_fwd": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, f32, f32, vp, i32, vp, vp, vp,
                                 vp]),
    "cilrs_bn_eval_fwd": (i32, [vp, i32, i32, vp, vp, vp, vp, f32, vp, i32, vp, vp, vp]),
    "cilrs_bn_bwd": (i32, [vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "cilrs_bn_bwd_frozen": (i32, [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp]),
    "cilrs_bn_bwd_pool_frozen": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "cilrs_saliency_map": (i32, [vp, C.c_long, C.c_long, C.c_long, C.c_long, i32, i32, i32,
                                 c_float_p, vp, vp, vp, vp]),
    "cilrs_attr_samples": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, u64, vp, vp]),
    "cilrs_attr_accumulate": (i32, [vp, C.c_long, C.c_long, C.c_long, C.c_long, i32, i32, i32, i32,
                                    i32, vp, vp]),
    "cilrs_attr_finalize": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, c_float_p, vp, vp, vp, vp]),
    "cilrs_attr_finalize_threads": (i32, []),
    "cilrs_adv_start": (i32, [vp, C.c_long, C.c_long, C.c_long, C.c_long, i32, i32, i32, f32,
                              c_float_p, u64, c_float_p, vp, C.c_long, C.c_long, C.c_long, C.c_long,
                              vp]),
    "cilrs_adv_step": (i32, [vp, vp, C.c_long, C.c_long, C.c_long, C.c_long, vp, C.c_long, C.c_long,
                             C.c_long, C.c_long, i32, i32, i32, f32, f32, c_float_p, vp, vp, vp,
                             C.c_long, C.c_long, C.c_long, C.c_long, c_float_p, vp]),
    "cilrs_adv_direction": (i32, [vp, vp, vp, vp, c_float_p, i32, i32, vp, vp, vp, vp, vp]),
    "cilrs_adv_quantize": (i32, [vp, C.c_long, C.c_long, C.c_long, C.c_long, vp, i32, i32, i32, vp,
                                 vp, vp]),
    "cilrs_adv_quantize_threads": (i32, []),
    "cilrs_adv_max_elements": (C.c_longlong, []),
    "cilrs_linear_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cilrs_linear_bwd": (i32, [vp, vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32,
                               vp]),
    "cilrs_maxpool_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "cilrs_maxpool_bwd": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
}

_lib = None


def lib():
    """Load (once) and return the bound library; raises if the HIP extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"CILRS HIP extension not built: {LIB_PATH} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make` in csrc/). "
            "There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        msg = lib().cilrs_last_error()
        raise RuntimeError("cilrs_hip: " + (msg.decode() if msg else f"error {rc}"))


def ptr(t):
    """Device (or host) pointer of a torch tensor, or None."""
    return None if t is None else C.c_void_p(t.data_ptr())
