"""ctypes binding of libgags_hip.so (C ABI: include/gags_raster.h).

The library is the product: there is NO fallback.  If it is missing or fails to load,
every op raises -- nothing silently routes to PyTorch or to the CPU oracle.
"""
import ctypes
import os
import subprocess

# torch must be imported BEFORE libgags_hip.so is dlopen'ed: the torch wheel bundles its own
# libamdhip64.so (soname libamdhip64.so.7) and resolves it by path.  If our library pulled in
# /opt/rocm's copy first, the process would hold two HIP runtimes and every launch on a torch
# pointer/stream would fail.  Loaded in this order, the dynamic linker binds our DT_NEEDED
# libamdhip64.so.7 to the runtime torch already loaded.
import torch  # noqa: F401  (load order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libgags_hip.so")

_vp, _i32, _i64, _f32, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double

# name -> (restype, argtypes); must list every symbol include/gags_raster.h declares
SIGNATURES = {
    "gags_abi_version": (_i32, []),
    "gags_strerror": (ctypes.c_char_p, [_i32]),
    "gags_device_count": (_i32, []),
    "gags_project_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _f32, _f32,
                                _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_project_fwd_raw": (_i32, [_i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _f32, _f32, _f32,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_project_bwd_raw": (_i32, [_i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp]),
    # N16: rasterize_mode "antialiased" (one more output / cotangent: the compensations) and absgrad
    "gags_project_fwd_aa": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _f32, _f32,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_project_bwd_aa": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp]),
    "gags_project_fwd_raw_aa": (_i32, [_i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _f32, _f32, _f32,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_project_bwd_raw_aa": (_i32, [_i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp]),
    "gags_raster_bwd_abs": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    # N17: camera pose gradients (flags, n, ..., v_viewmat, partials, partials_bytes) and the column-sum kernel behind them
    "gags_project_pose_partials": (_i64, [_i32]),
    "gags_project_bwd_pose": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_colsum_f32": (_i32, [_i64, _i32, _vp, _f32, _vp, _i32, _vp]),
    # N20: camera models (camera_model, flags, n, ...): the union of the projection entries' arguments
    "gags_project_fwd_cam": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _f32, _f32, _f32,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_project_bwd_cam": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    # N23: intrinsics gradients: gags_project_bwd_cam's arguments, then v_K, v_coeffs behind v_viewmat
    "gags_project_calib_partials": (_i64, [_i32]),
    "gags_project_bwd_calib": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_scan_scratch_bytes": (_i64, [_i32]),
    "gags_cumsum_i32": (_i32, [_i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_cumsum_gather_i32": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_read_i32": (_i32, [_vp, _vp, _vp]),
    "gags_depth_order_scratch_bytes": (_i64, [_i32]),
    "gags_depth_order": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_tile_emit": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "gags_tile_emit_cap": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "gags_sort_scratch_bytes": (_i64, [_i64]),
    "gags_sort_pairs": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_tile_offsets": (_i32, [_i64, _vp, _i32, _vp, _vp]),
    "gags_pack_isects": (_i32, [_i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_raster_fwd_scratch_bytes": (_i64, [_i64, _i32, _i32]),
    "gags_raster_fwd": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp,
                               _vp, _i64, _vp, _i32, _vp]),
    "gags_raster_bwd": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _i32, _vp]),
    "gags_bwd_rowmap_scratch_bytes": (_i64, [_i64]),
    "gags_bwd_rowmap_elems": (_i64, [_i64, _i32, _i32]),
    "gags_bwd_rowmap": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "gags_raster_bwd_geom_scratch_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32, _i64]),
    "gags_raster_bwd_geom": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64,
                                    _vp, _vp, _vp, _i64, _i32, _vp]),
    "gags_blended_mask": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "gags_bwd_staged_scratch_bytes": (_i64, [_i64, _i32, _i32]),
    "gags_raster_bwd_colors_staged": (_i32, [_i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp,
                                             _i64, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_raster_list_need": (_i32, [_i32, _i32, _i32, _vp, _vp, _i64, _vp, _i32, _vp, _vp]),
    "gags_trim_lists": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_trim_last_ids": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gags_raster_stats": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "gags_project_bwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp]),
    "gags_sh_fwd": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_sh_bwd": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_sh_bwd_dirs": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_ed_normalize": (_i32, [_i64, _i32, _vp, _vp, _vp]),
    "gags_adam_step": (_i32, [_i64, _vp, _vp, _vp, _vp, _f64, _f64, _f64, _f64, _i32, _vp]),
    "gags_pack_rows": (_i32, [_i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "gags_unpack_rows": (_i32, [_i64, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "gags_compact_mask_scratch_bytes": (_i64, [_i32]),
    "gags_compact_mask": (_i32, [_i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "gags_compact_mask_pos": (_i32, [_i32, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_dot_scratch_bytes": (_i64, []),
    "gags_dot_f32": (_i32, [_i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    # include/gags_next.h
    "gags_trained_seg": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp]),
    "gags_entropy_fwd": (_i32, [_i64, _vp, _vp, _vp]),
    "gags_entropy_bwd": (_i32, [_i64, _vp, _f32, _vp, _vp]),
    "gags_entropy_bwd_dev": (_i32, [_i64, _vp, _vp, _vp, _vp]),
    "gags_segment_stats": (_i32, [_i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "gags_segment_stats_multi": (_i32, [_i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "gags_segment_stats_runs_copies": (_i32, [_i64, _i32, _i32, _i32]),
    "gags_segment_stats_runs": (_i32, [_i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "gags_segment_loss": (_i32, [_i32, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_region_var_bwd_layout": (_i32, [_i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "gags_region_var_bwd_add": (_i32, [_i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gags_region_var_bwd": (_i32, [_i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "gags_gather_seg_coef": (_i32, [_i64, _vp, _i32, _vp, _vp, _vp]),
    "gags_sam_clip_feature": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_sam_clip_feature_max": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_sam_clip_feature_bwd_scale": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gags_distill_l1_map_fwd": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "gags_distill_l1_map_bwd": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "gags_decoder_head_distill_fwd": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_head_distill_bwd": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_head_distill_bwd_f32": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_pack_input": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp]),
    "gags_decoder_pack_layer": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_pack_layers": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_layer": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_wgrad_scratch_bytes": (_i64, [_i64, _i32, _i32]),
    "gags_decoder_wgrad": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_decoder_wgrad_out": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp]),
    "gags_decoder_head_bwd": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "gags_decoder_unpack_grad": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp]),
    "gags_decoder_head": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "gags_decoder_fwd_fused": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_bwd_fused": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_bwd_fused_scaled": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_scale_decoder_fwd_fused": (_i32, [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_scale_decoder_fwd_fused_head": (_i32, [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_softmax_head_bwd_y": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "gags_scale_decoder_bwd_fused": (_i32, [_i64, _vp, _vp, _vp, _vp, _vp]),
    "gags_decoder_layer_exact": (_i32, [_i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "gags_decoder_layer_split": (_i32, [_i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gags_decoder_wgrad_split": (_i32, [_i64, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp]),
    "gags_decoder_wgrad_exact_scratch_bytes": (_i64, [_i64, _i32, _i32]),
    "gags_decoder_wgrad_exact": (_i32, [_i64, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    "gags_decoder_head_bwd_exact": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp]),
    # the "f16" decoder tier: the same kernels with IEEE half operands (include/gags_next.h), same signatures
    **{name + "_h16": None for name in ("gags_decoder_pack_layer", "gags_decoder_pack_layers", "gags_decoder_pack_input", "gags_decoder_layer", "gags_decoder_head",
                                        "gags_decoder_wgrad_scratch_bytes", "gags_decoder_wgrad", "gags_decoder_wgrad_out",
                                        "gags_decoder_head_bwd",
                                        "gags_decoder_unpack_grad", "gags_decoder_fwd_fused", "gags_decoder_bwd_fused", "gags_decoder_bwd_fused_scaled",
                                        "gags_scale_decoder_fwd_fused", "gags_scale_decoder_bwd_fused", "gags_scale_decoder_fwd_fused_head",
                                        "gags_softmax_head_bwd_y", "gags_decoder_query_fused")},
    "gags_pow2_scale": (_i32, [_vp, _f32, _f32, _vp, _vp]),
    "gags_decoder_head_distill_bwd_h16": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_relevancy": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gags_relevancy_activate_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "gags_relevancy_activate": (_i32, [_i32, _i32, _i32, _vp, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_point_relevancy_mask_scratch_bytes": (_i64, [_i32, _i64]),
    "gags_point_relevancy_mask": (_i32, [_i32, _i64, _vp, _f32, _vp, _vp, _vp, _i64, _vp]),
    "gags_point_mask_smooth_scratch_bytes": (_i64, [_i32, _i64]),
    "gags_point_mask_smooth": (_i32, [_i32, _i64, _vp, _vp, _f64, _i32, _vp, _vp, _vp, _i64, _vp]),
    "gags_depthsample_scratch_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "gags_depthsample_map": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gags_depthsample_scatter": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _i64, _vp]),
    # N22: ... for a rig of any camera models (cam_models: a HOST int32 array or NULL, radial_coeffs: device [C, 4] or NULL)
    "gags_rig_depth_scratch_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "gags_rig_depth_map": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _vp, _i64,
                                  _vp]),
    "gags_rig_depth_scatter": (_i32, [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _i64,
                                      _vp]),
    # N7: the photometric loss of the RGB stage
    "gags_photometric_partials": (_i64, [_i32, _i32, _i32]),
    "gags_photometric_fwd": (_i32, [_i32, _i32, _i32, _i32, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _f64, _f64, _f64,
                                    _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_photometric_bwd": (_i32, [_i32, _i32, _i32, _i32, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp,
                                    _i64, _i64, _i64, _vp]),
    # N24: bilateral grid colour correction (csrc/bilagrid.hip): (L, gh, gw, h, w, grid, rgb + 3 strides, ...)
    "gags_bilagrid_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "gags_bilagrid_slice_fwd": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "gags_bilagrid_slice_bwd": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp,
                                       _vp, _i64, _vp]),
    "gags_bilagrid_tv_partials": (_i64, [_i32, _i32, _i32, _i32]),
    "gags_bilagrid_tv_fwd": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "gags_bilagrid_tv_bwd": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    # N8: adaptive density control (csrc/densify.hip)
    "gags_densify_stats": (_i32, [_i32, _vp, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp]),
    "gags_densify_decide": (_i32, [_i32, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _vp]),
    "gags_densify_plan": (_i32, [_i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "gags_densify_gather": (_i32, [_i64, _vp, _vp, _i32, _vp, _vp]),
    "gags_densify_children": (_i32, [_i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "gags_reset_opacity": (_i32, [_i64, _vp, _vp, _vp, _vp]),
    # N9: scene initialisation from a point cloud (csrc/knn.hip)
    "gags_knn3_dist2_scratch_bytes": (_i64, [_i64]),
    "gags_knn3_dist2": (_i32, [_i64, _vp, _vp, _vp, _i64, _vp]),
    # N10: SAM mask post-processing on bit-packed masks (csrc/sam_masks.hip)
    "gags_masks_max_count": (_i32, []),
    "gags_masks_pair_chunk_words": (_i32, []),
    "gags_masks_pack": (_i32, [_i32, _i64, _vp, _vp, _vp, _vp]),
    "gags_masks_pairs": (_i32, [_i32, _i64, _vp, _vp, _vp]),
    "gags_masks_colmax": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp]),
    "gags_masks_paint": (_i32, [_i32, _i64, _vp, _i32, _vp, _i32, _vp, _vp]),
    "gags_masks_nms_scratch_bytes": (_i64, [_i32, _i64]),
    "gags_masks_nms_colmax": (_i32, [_i32, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    # N11: PCA colouring of a feature map (csrc/featurevis.hip)
    "gags_featvis_row_chunk": (_i32, []),
    "gags_featvis_moments_scratch_bytes": (_i64, [_i32, _i64]),
    "gags_featvis_moments": (_i32, [_i32, _i64, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    "gags_featvis_project": (_i32, [_i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "gags_featvis_select_scratch_bytes": (_i64, [_i32]),
    "gags_featvis_select": (_i32, [_i64, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _vp]),
    "gags_featvis_colour": (_i32, [_i64, _vp, _f32, _f32, _vp, _vp, _vp]),
    # N12: query images and loss maps (csrc/queryvis.hip)
    "gags_query_images_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "gags_query_images": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _i64, _vp]),
    "gags_query_colour": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_feature_loss_maps": (_i32, [_i32, _i64, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    # N13: crop statistics for SAM's depth-aware prompt grids (csrc/promptgrid.hip)
    "gags_promptgrid_scratch_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "gags_promptgrid_stats": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    # N14: CLIP tiles from SAM masks (csrc/tilecut.hip)
    "gags_tilecut_side": (_i32, []),
    "gags_tilecut": (_i32, [_i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gags_tilecut_boxes": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp]),
    # N15: the query head, CNN_decoder + relevancy in one kernel (csrc/decoder_query.hip)
    "gags_decoder_query_fused": (_i32, [_i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    # N18: MCMC density control (csrc/mcmc.hip)
    "gags_mcmc_sample": (_i32, [_i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "gags_mcmc_relocation": (_i32, [_i32, _vp, _i32, _f64, _vp, _vp, _vp]),
    "gags_mcmc_copy_rows": (_i32, [_i64, _vp, _vp, _i32, _i32, _vp, _vp]),
    "gags_mcmc_noise": (_i32, [_i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp]),
    "gags_mcmc_reg_partials": (_i64, [_i32]),
    "gags_mcmc_reg_fwd": (_i32, [_i32, _vp, _vp, _f32, _f32, _vp, _i64, _vp, _vp]),
    "gags_mcmc_reg_bwd": (_i32, [_i32, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp]),
    # N19: row-selective Adam, all tensors of a step in one launch (csrc/optim.hip)
    "gags_adam_tensor_bytes": (_i64, []),
    "gags_adam_step_rows": (_i32, [_i64, ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp]),
}

for _name in [k for k, v in SIGNATURES.items() if v is None]:  # (a twin's signature is its bf16 counterpart's)
    SIGNATURES[_name] = SIGNATURES[_name[:-4]]

GAGS_BWD_COLORS_ONLY = 1
GAGS_FWD_NO_MFMA = 2
GAGS_FWD_ONLY_WEIGHTS, GAGS_FWD_ONLY_FEATURES = 512, 1024  # C flags: one kernel of the split forward per call (per-kernel timing)
GAGS_RECS_BY_GAUSSIAN = 256  # C flag: `packed` is the per-Gaussian record table (gags_pack_isects with packed = NULL)
GAGS_BWD_ATOMIC = 4  # python-side: use the atomic colours-only backward instead of the staged one
GAGS_FEAT_F16 = 32  # forward: colors is an fp16 table (include/gags_raster.h)
GAGS_BWD_F32MFMA = 64  # python-side: staged backward contracts with v_mfma_f32_32x32x2_f32 (round 1-2's kernel) instead of the
#                        default fp32-equivalent split operands on the 16-bit matrix cores (csrc/raster_bwd_rows.hip)
GAGS_BWD_BLOCKWAVES = 4096  # python-side: the staged backward's rows kernel in round 4's shape (a wave per 8x8 pixel block, rows
#                             merged in LDS: GAGS_STAGED_BLOCKWAVES) instead of the default (a wave per 32 channels, rows merged in the accumulators)
GAGS_BWD_EXACT_WEIGHTS = 8192  # python-side: the default rows kernel with the weights as THREE fp16 terms (exact) and five product terms
#                                (GAGS_STAGED_EXACT_WEIGHTS) instead of two terms / three product terms: 1.60e-7 instead of 1.68e-7 of float64, 1.33x the time
GAGS_BWD_F16SPLIT = 0   # (round 2's opt-in flag: that kernel, made exact, is the default now)
GAGS_FWD_F16MFMA = 128  # python-side: fp16 feature table + D % 128 == 0: feature pass on the 16-bit matrix cores (opt-in; C flag 64)
GAGS_FWD_F16MFMA_C = 64  # C flag: the header's GAGS_FWD_F16MFMA.  Two constants because the public request bit above was given
#                          128 (64 was taken by the python-side GAGS_BWD_F32MFMA); raster_route._fwd_flags translates
GAGS_FWD_EXACT = 2048  # fp32 table, D >= 128: feature pass on v_mfma_f32_32x32x2_f32, bit-identical to the sequential fmaf chain (the
#                        oracle); default: 16-bit matrix cores on operands split into three bf16 terms (include/gags_raster.h)
GAGS_FWD_FUSED = 8  # python-side: single-kernel matrix-core forward (no scratch) instead of weights + features
# `stage` of gags_raster_bwd_colors_staged (include/gags_raster.h; tests/test_abi_cpu.py compares the two): which of the three
# stages a call runs, OR-ed with the bits that select a rows kernel, the output dtype and how v_colors / the scratch are used
GAGS_STAGE_ALL, GAGS_STAGE_ROWS, GAGS_STAGE_SORT, GAGS_STAGE_REDUCE, GAGS_STAGE_MASK = 0, 1, 2, 3, 15
GAGS_STAGED_F32MFMA, GAGS_STAGED_OUT_F16, GAGS_STAGED_PREZEROED = 32, 64, 128
GAGS_STAGED_RANGE_SCRATCH, GAGS_STAGED_BLOCKWAVES, GAGS_STAGED_EXACT_WEIGHTS = 256, 512, 1024
GAGS_KIND_KEEP, GAGS_KIND_CLONE, GAGS_KIND_CHILD_A, GAGS_KIND_CHILD_B = 0, 1, 2, 3  # `kind` of gags_densify_plan
GAGS_GATHER_MAX_DESC, GAGS_GATHER_COPY, GAGS_GATHER_MOMENT = 24, 0, 1  # gags_densify_gather, gags_mcmc_copy_rows
GAGS_MCMC_MAX_RATIO = 51  # gags_mcmc_relocation clamps a ratio to [1, this]


class GatherDesc(ctypes.Structure):
    """gags_gather_desc of include/gags_next.h."""
    _fields_ = [("in_", _vp), ("out", _vp), ("row_floats", ctypes.c_int32), ("mode", ctypes.c_int32)]


class AdamTensor(ctypes.Structure):
    """gags_adam_tensor of include/gags_raster.h (gags_adam_tensor_bytes() is its size on the C side)."""
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("width", _i64),
                ("lr", _f64), ("beta1", _f64), ("beta2", _f64), ("eps", _f64)]


GAGS_ADAM_MAX_TENSORS, GAGS_ADAM_SKIP_ZERO_ROWS, GAGS_ADAM_NO_BIAS_CORRECTION = 8, 1, 2  # gags_adam_step_rows

GAGS_GEOM_F32MFMA = 32  # `flags` of gags_raster_bwd_geom: the fp32 matrix instructions (what GAGS_BWD_F32MFMA asks of that kernel)
GAGS_POSE_RAW, GAGS_POSE_AA = 1, 2  # `flags` of gags_project_bwd_pose
GAGS_CAM_PINHOLE, GAGS_CAM_ORTHO, GAGS_CAM_FISHEYE = 0, 1, 2  # `camera_model` of gags_project_fwd_cam / gags_project_bwd_cam
GAGS_PROJ_RAW, GAGS_PROJ_AA, GAGS_PROJ_POSE = 1, 2, 4  # their `flags`
GAGS_CALIB_PARTIAL_FLOATS = 22  # floats per row of gags_project_bwd_calib's partials (N23): 12 pose, 6 K, 4 coefficients
GAGS_PROJ_KB = 32  #... and (N21, fisheye only): K is 13 floats, the 3 x 3 matrix then the distortion coefficients k1 .. k4
CAMERA_MODELS = {"pinhole": GAGS_CAM_PINHOLE, "ortho": GAGS_CAM_ORTHO, "fisheye": GAGS_CAM_FISHEYE}  # rasterization(camera_model=)
GAGS_GEOM_ABSGRAD = 64  # `flags` of gags_raster_bwd_geom: columns 6, 7 of v_geo carry absgrad (rasterization(absgrad=True))

_lib = None


class GagsLibraryError(RuntimeError):
    pass


def build(verbose=False):
    """Compile gags_amd/csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC, "-j8", "libgags_hip.so"], stdout=out)
    return LIB_PATH


def load():
    """dlopen the library and type every entry point.  Raises GagsLibraryError when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GagsLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C gags_amd/csrc`.  gags_amd has no CPU / PyTorch fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise GagsLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise GagsLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().gags_strerror(code)
        raise RuntimeError(f"{what} failed: {msg.decode() if msg else code} ({code})")


def ptr(t):
    """Raw device pointer of a tensor (or NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# What every binding module needs around a call; used as attributes of this module (_lib.scratch(...)) so that a test
# can substitute one.
def stream(device=None):
    """The current HIP stream of `device` (default: the current device) as the `void *stream` of the C entries."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_gpu(module, *tensors):
    """Refuse anything that is not a GPU tensor, in the name of gags_amd.<module>."""
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"gags_amd.{module}: tensors must live on the GPU (there is no CPU path)")


def scratch(nbytes, device):
    """A uint8 buffer for a C entry's `scratch`; the caller passes the library's own byte count as `scratch_bytes`."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
