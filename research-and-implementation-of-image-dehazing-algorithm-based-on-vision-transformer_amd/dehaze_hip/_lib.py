"""ctypes binding of libdehaze_hip.so (C-ABI declared in include/dehaze_hip.h).

There is NO fallback: if the shared object is missing the import of the product fails loudly with
the build instruction; nothing here routes to PyTorch eager or to the CPU oracle.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DHZ_LIB_PATH") or os.path.join(_HERE, "libdehaze_hip.so")   # override: A/B of two builds

c_f = ctypes.c_void_p      # device float*
c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_l = ctypes.c_int64
c_fl = ctypes.c_float

# name -> argtypes  (return type is int unless listed in _RESTYPE)
SIGNATURES = {
    "dhz_abi_version": [],
    "dhz_last_error": [],
    "dhz_build_id": [],
    "dhz_set_reserved_cus": [ctypes.c_int],
    "dhz_gelu_fwd_dt": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p],
    "dhz_gelu_bwd_dt": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p],
    "dhz_get_reserved_cus": [],
    "dhz_set_deterministic": [ctypes.c_int],
    "dhz_get_deterministic": [],
    "dhz_set_det_workspace": [ctypes.c_void_p, ctypes.c_size_t],
    "dhz_grid_cus": [],
    "dhz_ps_attn_fwd": [c_f, c_f, c_f, c_i, c_p, c_f, c_f, c_f, c_i, c_p, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_bwd_parts": [c_i, c_i],
    "dhz_ps_attn_bwd_parts_d": [c_i, c_i, c_i],
    "dhz_ps_attn_bwd": [c_f, c_f, c_f, c_i, c_f, c_f, c_p, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_fused_attn_prepack": [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_p],
    "dhz_fused_window_attn_fwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p,
                                  c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_fused_window_attn_fwd6": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p,
                                   c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_fused_attn_prepack6": [c_f, c_f, c_f, c_f, c_p, c_i, c_p],
    "dhz_fused_attn_prepack6_multi": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p],
    "dhz_fused_attn_bwd_parts": [c_i],
    "dhz_fused_attn_bwd_prepack": [c_f, c_f, c_f, c_f, c_f, c_i, c_p],
    "dhz_fused_window_attn_bwd": [c_f] * 11 + [c_f] * 12 + [c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_dense_attn_fwd": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_fl, c_p],
    "dhz_dense_attn_bwd": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_fl, c_p],
    "dhz_bias_gather": [c_f, c_f, c_i, c_p],
    "dhz_bias_gather_multi": [c_p, c_p, c_p, c_i, c_p],
    "dhz_fused_attn_prepack_multi": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p],
    "dhz_bias_table_grad": [c_f, c_i, c_f, c_i, c_i, c_p],
    "dhz_bias_table_grad_multi": [c_p, c_p, c_p, c_p, c_i, c_p],
    "dhz_shift_mask": [c_f, c_i, c_i, c_i, c_p],
    "dhz_thin_conv3x3_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_thin_conv3x3_dgrad": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_conv3x3_in3_blocked": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_thin_conv3x3_dgrad_blocked": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_thin_conv3x3_wgrad": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_l1_pair_fwd": [c_f, c_f, c_f, c_f, c_l, c_p],
    "dhz_l1_pair_bwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_p],
    "dhz_contrast_combine_fwd": [c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_p],
    "dhz_contrast_combine_bwd": [c_f, c_f, c_i, c_i, c_f, c_f, c_f, c_f, c_p],
    "dhz_crop_augment_pair": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd_prepack": [c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_winograd_conv3x3": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd43_prepack": [c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_winograd43_conv3x3": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd43_conv3x3_pool": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd_conv3x3_slices": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd43_conv3x3_slices": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd_slices": [c_i, c_i, c_i, c_i, c_i],
    # the F(2x2) convolution on maps of any size (ragged blocks; sixteen 4 x 4 images per block)
    "dhz_winograd_conv3x3_any": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd_conv3x3_any_slices": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_winograd_slices_any": [c_i, c_i, c_i, c_i, c_i],
    "dhz_winograd_any_blocks": [c_i, c_i, c_i],
    "dhz_maxpool2x2_blocked_fwd": [c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_maxpool2x2_blocked_bwd": [c_f, c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_layout_blocked8": [c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_p],
    "dhz_leff_fused_fwd": [c_f] * 16 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_fused_fwd6": [c_f] * 15 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_prepack6": [c_f, c_f, c_p, c_i, c_p],
    "dhz_linear_fwd": [c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_dgrad": [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_input_proj_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_p],
    "dhz_input_proj_bwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_p],
    "dhz_conv4s2_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_conv4s2_dgrad": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_conv4s2_wgrad": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_input_proj_fwd_dt": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_i, c_p],
    "dhz_input_proj_bwd_dt": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_i, c_p],
    "dhz_thin_conv3x3_fwd_dt": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_thin_conv3x3_dgrad_dt": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_thin_conv3x3_wgrad_dt": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_vgg_prepack_bf16": [c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_vgg_conv3x3_bf16": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_maxpool2x2_nhwc_bf16_fwd": [c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_maxpool2x2_nhwc_bf16_bwd": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_l1_pair_fwd_bf16": [c_f, c_f, c_f, c_f, c_l, c_p],
    "dhz_l1_pair_bwd_bf16": [c_f, c_f, c_f, c_f, c_f, c_l, c_p],
    "dhz_im2col_k4s2_bf16": [c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_col2im_k4s2_bf16": [c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_fwd_split": [c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_dgrad_split": [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_wgrad_split": [c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_i, c_i, c_p],
    "dhz_linear_bwd_pair": [c_f, c_i, c_f, c_i, c_p, c_p, c_p, c_f, c_i, c_i, c_i, c_i, c_f, c_f, c_p],
    "dhz_linear_bwd_pair_grid": [c_i, c_i, c_i],
    "dhz_linear_fwd_split6": [c_f, c_i, c_p, c_p, c_p, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_dgrad_split6": [c_f, c_i, c_p, c_p, c_p, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_fwd_split6_res": [c_f, c_i, c_p, c_p, c_p, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_fwd_split_res": [c_f, c_i, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_fwd_bf16_res": [c_f, c_i, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_dgrad_split_scaled": [c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ln_partition_bwd_lay2": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_i, c_p],
    "dhz_ln_partition_bwd_lay": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_split3_planes": [c_f, c_l, c_p, c_p, c_p, c_p],
    "dhz_split3_planes_t": [c_f, c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "dhz_linear_fwd_bf16": [c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_bf16_transpose_batched": [c_f, c_p, c_p, c_i, c_i, c_p],
    "dhz_linear_dgrad_bf16": [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_wgrad_bf16": [c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p],
    "dhz_ln_partition_fwd_dt": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ln_partition_bwd_dt": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_reverse_residual_fwd_dt": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_reverse_residual_bwd_dt": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_dwconv_fwd_dt": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_dwconv_bwd_dt": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_dwconv_bwd_scaled_dt": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_dwconv_bwd_dy": [c_f, c_i, c_p, c_p, c_p, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_fwd_dt": [c_f, c_f, c_f, c_i, c_p, c_f, c_f, c_f, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_bwd_dt": [c_f, c_f, c_f, c_i, c_f, c_f, c_p, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_linear_wgrad": [c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_f, c_p],
    "dhz_linear_wgrad_rs": [c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_i, c_p],
    "dhz_linear_wgrad_multi": [c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p],
    "dhz_ln_partition_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ln_partition_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_reverse_residual_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_reverse_residual_bwd": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_dwconv_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_leff_dwconv_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_charbonnier_fwd": [c_f, c_f, c_f, c_f, c_l, c_fl, c_i, c_p],
    "dhz_charbonnier_bwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_fl, c_fl, c_i, c_p],
    "dhz_adamw_step": [c_f, c_f, c_f, c_f, c_l, c_fl, c_fl, c_fl, c_fl, c_fl, c_i, c_fl, c_p],
    "dhz_comm_unique_id": [c_p],
    "dhz_comm_init": [c_p, c_i, c_i, c_p],
    "dhz_comm_allreduce_sum_f32": [c_p, c_f, c_l, c_p],
    "dhz_comm_destroy": [c_p],
    "dhz_adamw_step_shadow": [c_f, c_f, c_f, c_f, c_f, c_l, c_fl, c_fl, c_fl, c_fl, c_fl, c_i, c_fl, c_p],
    # win x win windows (win = 4 or 8): the entry of the same name without `_w` plus `win`
    "dhz_ps_attn_fwd_w": [c_f, c_f, c_f, c_i, c_p, c_f, c_f, c_f, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_bwd_parts_w": [c_i, c_i, c_i, c_i],
    "dhz_ps_attn_bwd_w": [c_f, c_f, c_f, c_i, c_f, c_f, c_p, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_dense_attn_fwd_w": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_fl, c_i, c_p],
    "dhz_dense_attn_bwd_w": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_fl, c_i, c_p],
    "dhz_ln_partition_fwd_w": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ln_partition_bwd_w": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_reverse_residual_fwd_w": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_reverse_residual_bwd_w": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_shift_mask_w": [c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_bias_gather_w": [c_f, c_f, c_i, c_i, c_p],
    "dhz_bias_table_grad_w": [c_f, c_i, c_f, c_i, c_i, c_i, c_p],
    # padding mask of any-size evaluation as one uint64 per window: the entry of the same name without `_pad` plus `pad` behind `mask`
    "dhz_pad_window_bits": [c_f, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_fwd_dt_pad": [c_f, c_f, c_f, c_i, c_p, c_f, c_f, c_p, c_f, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_bwd_dt_pad": [c_f, c_f, c_f, c_i, c_f, c_f, c_p, c_p, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_fwd_w_pad": [c_f, c_f, c_f, c_i, c_p, c_f, c_f, c_p, c_f, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ps_attn_bwd_w_pad": [c_f, c_f, c_f, c_i, c_f, c_f, c_p, c_p, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_fused_window_attn_fwd_pad": [c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_f, c_f, c_p, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    # dense 3x3 convolution of the UNet baseline on the channel-blocked layout: LeakyReLU in the Winograd store, weight gradient
    "dhz_winograd_conv3x3_act": [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_tokens_to_blocked8": [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_blocked8_to_tokens": [c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_p],
    "dhz_conv3x3_wgrad_workspace_bytes": [c_i, c_i, c_i, c_i, c_i],
    "dhz_conv3x3_wgrad_parts": [c_i, c_i, c_i, c_i, c_i],
    "dhz_conv4s2_tile": [c_i, c_i, c_i, c_i, c_i, c_i],
    # Downsample on the six-term plane kernels (csrc/split6_gemm.hip)
    "dhz_conv4s2_prepack6": [c_f, c_p, c_p, c_i, c_i, c_p],
    "dhz_conv4s2_fwd6": [c_f, c_p, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_conv4s2_dgrad6": [c_f, c_p, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_conv4s2_tile6": [c_i, c_i, c_i, c_i, c_i, c_i],
    "dhz_linear_tile": [c_i, c_i],
    "dhz_linear_split6_tile": [c_i, c_i, c_i, c_i],
    "dhz_conv3x3_wgrad": [c_f, c_f, c_f, c_f, c_f, ctypes.c_size_t, c_i, c_i, c_i, c_i, c_i, c_p],
    # FFA-Net's channel / pixel attention on the channel-blocked layout (csrc/ffa_attn.hip)
    "dhz_ffa_workspace_bytes": [c_i, c_i, c_i, c_i],
    "dhz_ffa_ca_fwd": [c_f] * 11 + [ctypes.c_size_t, c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_gate_pa_fwd": [c_f] * 10 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_gate_pa_bwd_a": [c_f] * 11 + [ctypes.c_size_t, c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_ca_bwd": [c_f, ctypes.c_size_t] + [c_f] * 14 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_gate_pa_bwd_b": [c_f] * 6 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_add": [c_f, c_f, c_f, c_l, c_p],
    # the same attention entries and the dense weight gradient on maps of any size (ragged tails; FFA-Net on whole images)
    "dhz_ffa_workspace_bytes_any": [c_i, c_i, c_i, c_i],
    "dhz_ffa_add_any": [c_f, c_f, c_f, c_l, c_p],
    "dhz_ffa_ca_fwd_any": [c_f] * 11 + [ctypes.c_size_t, c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_gate_pa_fwd_any": [c_f] * 10 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_gate_pa_bwd_a_any": [c_f] * 11 + [ctypes.c_size_t, c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_ca_bwd_any": [c_f, ctypes.c_size_t] + [c_f] * 14 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_gate_pa_bwd_b_any": [c_f] * 6 + [c_i, c_i, c_i, c_i, c_p],
    "dhz_conv3x3_wgrad_workspace_bytes_any": [c_i, c_i, c_i, c_i, c_i],
    "dhz_conv3x3_wgrad_parts_any": [c_i, c_i, c_i, c_i, c_i],
    "dhz_conv3x3_wgrad_any": [c_f, c_f, c_f, c_f, c_f, ctypes.c_size_t, c_i, c_i, c_i, c_i, c_i, c_p],
    "dhz_ffa_relu_bwd_add": [c_f, c_f, c_f, c_f, c_f, c_l, c_p],
    # squared-error taps of FFA-Net's perceptual loss, pooling backward of a map that is a tap too (csrc/perceptual.hip)
    "dhz_mse_pair_fwd": [c_f, c_f, c_f, c_l, c_p],
    "dhz_mse_pair_bwd": [c_f, c_f, c_f, c_f, c_l, c_i, c_p],
    "dhz_maxpool2x2_blocked_bwd_add": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_p],
    # whole images: the poolings and the L1 mean on any size, the feed for h x w crops
    "dhz_maxpool2x2_blocked_fwd_any": [c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_maxpool2x2_blocked_bwd_any": [c_f, c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_maxpool2x2_blocked_bwd_add_any": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_p],
    "dhz_l1_pair_fwd_any": [c_f, c_f, c_f, c_f, c_l, c_p],
    "dhz_l1_pair_bwd_any": [c_f, c_f, c_f, c_f, c_f, c_l, c_p],
    "dhz_crop_augment_pair_rect": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_p],
    # the feed for pools of images of any sizes: (gt pool, hazy pool, int64 descriptor rows, out gt, out hazy, host norm[6] | NULL, n, h, w)
    "dhz_crop_augment_pair_ragged": [c_p, c_p, c_p, c_f, c_f, c_p, c_i, c_i, c_i, c_p],
    # SSIM / squared error of image pairs in float64 (csrc/metrics.hip)
    "dhz_ssim_pair_workspace_bytes": [c_i, c_i, c_i, c_i],
    "dhz_ssim_pair": [c_p, c_p, c_f, c_l, c_l, c_f, c_l, c_l, c_i, c_i, c_i, c_i, c_i, c_f, ctypes.c_double, c_i, ctypes.c_double,
                      ctypes.c_double, ctypes.c_double, c_i, c_p, ctypes.c_size_t, c_p],
    # SSIM as a training loss: 1 - mean(S) and its gradient with respect to the prediction (csrc/ssim_loss.hip)
    "dhz_ssim_loss_workspace_bytes": [c_i, c_i, c_i, c_i, c_i],
    "dhz_ssim_loss_fwd": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_i, ctypes.c_double, ctypes.c_double, c_i, c_i, c_p,
                          ctypes.c_size_t, c_p],
    "dhz_ssim_loss_bwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_i, ctypes.c_double, ctypes.c_double, c_i, c_p,
                          ctypes.c_size_t, c_p],
}
_RESTYPE = {"dhz_last_error": ctypes.c_char_p, "dhz_build_id": ctypes.c_char_p, "dhz_conv3x3_wgrad_workspace_bytes": ctypes.c_size_t,
            "dhz_ffa_workspace_bytes": ctypes.c_size_t, "dhz_conv3x3_wgrad_workspace_bytes_any": ctypes.c_size_t,
            "dhz_ffa_workspace_bytes_any": ctypes.c_size_t, "dhz_ssim_pair_workspace_bytes": ctypes.c_size_t,
            "dhz_ssim_loss_workspace_bytes": ctypes.c_size_t}

_lib = None


class DehazeHipError(RuntimeError):
    pass


def load():
    """Load the shared object (once).  Raises ImportError with the build recipe if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is mandatory (there is no PyTorch/CPU fallback). "
            "Build it with `python __graft_entry__.py build` or `csrc/build.sh` (hipcc --offload-arch=gfx950).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch: fail loudly
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, ctypes.c_int)
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().dhz_last_error()
        raise DehazeHipError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def call(name, *args):
    check(getattr(load(), name)(*args), name)
