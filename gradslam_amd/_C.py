"""ctypes binding of libgradslam_hip.so (include/gradslam_hip.h).

The HIP library is the product: there is NO CPU or PyTorch fallback.  `lib()` raises if the
shared object is missing, and every wrapper raises if it is handed a tensor that does not live
on a HIP device.  torch is used only for device memory, streams and dtype plumbing.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# GRADSLAM_HIP_LIB: another build of the same library (A/B runs of an experimental build on one GPU box); it must export
# the same symbols and ABI version, and there is still no fallback if it is missing
LIB_PATH = os.environ.get("GRADSLAM_HIP_LIB") or os.path.join(_HERE, "csrc", "libgradslam_hip.so")
if os.environ.get("GRADSLAM_HIP_LIB"):   # (a bench line must not come from an experimental build unnoticed)
    import warnings
    warnings.warn("GRADSLAM_HIP_LIB overrides the product library: %s" % LIB_PATH, RuntimeWarning)
# knobs of engines that were measured, lost and removed: setting one must not pass silently
RETIRED_KNOBS = ("GRADSLAM_HIP_ICP_PERSIST", "GRADSLAM_HIP_ICP_PERSIST_TIMELINE", "GRADSLAM_HIP_ICP_FAR")
if any(k in os.environ for k in RETIRED_KNOBS):
    import warnings
    warnings.warn("retired knobs are set and ignored: %s (their engines were removed; the one ICP solve path runs)"
                  % ", ".join(k for k in RETIRED_KNOBS if k in os.environ), RuntimeWarning)
ABI_VERSION = 3

_lib = None

_vp, _i64, _i32, _f = C.c_void_p, C.c_int64, C.c_int, C.c_float


class IcpParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("numiters", C.c_int), ("damp", C.c_float),
                ("dist_thresh", C.c_float), ("lambda_max", C.c_float), ("B", C.c_float),
                ("B2", C.c_float), ("nu", C.c_float)]


class MapView(C.Structure):
    """gs_map_view: one sequence's capacity-backed surfel store as the batched entry points see it."""
    _fields_ = [("points", C.c_void_p), ("normals", C.c_void_p), ("colors", C.c_void_p), ("ccounts", C.c_void_p),
                ("capacity", C.c_int64), ("n_bound", C.c_int64), ("n_dev", C.c_void_p)]


class LocalizeSeq(C.Structure):
    _fields_ = [("vertex", C.c_void_p), ("depth", C.c_void_p), ("K16", C.c_void_p), ("prev_pose16", C.c_void_p),
                ("map", MapView), ("out_pose16", C.c_void_p), ("scratch", C.c_void_p)]


class UpdateSeq(C.Structure):
    _fields_ = [("map", MapView), ("vertex", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p),
                ("rgb", C.c_void_p), ("alpha", C.c_void_p), ("pose16", C.c_void_p), ("K16", C.c_void_p),
                ("gvertex", C.c_void_p), ("gnormal", C.c_void_p), ("best_pix", C.c_void_p),
                ("new_count_out", C.c_void_p), ("scratch", C.c_void_p)]


class StepSeq(C.Structure):
    """gs_step_seq: one sequence's part of gs_pointfusion_step_batch_f32."""
    _fields_ = [("depth", C.c_void_p), ("rgb", C.c_void_p), ("K16", C.c_void_p), ("prev_pose16", C.c_void_p),
                ("out_pose16", C.c_void_p), ("vertex", C.c_void_p), ("normal", C.c_void_p), ("alpha", C.c_void_p),
                ("gvertex", C.c_void_p), ("gnormal", C.c_void_p), ("best_pix", C.c_void_p),
                ("new_count_out", C.c_void_p), ("map", MapView), ("loc_scratch", C.c_void_p),
                ("upd_scratch", C.c_void_p)]


class RenderSeq(C.Structure):
    """gs_render_seq: one map and its L views for gs_render_map_dc_f32."""
    _fields_ = [("map", MapView), ("poses16", C.c_void_p), ("K16", C.c_void_p), ("depth", C.c_void_p),
                ("color", C.c_void_p), ("normal", C.c_void_p), ("confidence", C.c_void_p), ("index", C.c_void_p),
                ("scratch", C.c_void_p)]


class RenderBackwardSeq(C.Structure):
    """gs_render_backward_seq: one map, its L views, the saved index image, upstream adjoints and outputs."""
    _fields_ = [("map", MapView), ("poses16", C.c_void_p), ("K16", C.c_void_p), ("index", C.c_void_p),
                ("depth_bar", C.c_void_p), ("color_bar", C.c_void_p), ("normal_bar", C.c_void_p),
                ("confidence_bar", C.c_void_p), ("points_bar", C.c_void_p), ("normals_bar", C.c_void_p),
                ("colors_bar", C.c_void_p), ("ccounts_bar", C.c_void_p), ("poses_bar", C.c_void_p),
                ("scratch", C.c_void_p)]


class PruneSeq(C.Structure):
    """gs_prune_seq: one map, its destination buffers and controls for gs_prune_map_dc_f32."""
    _fields_ = [("points", C.c_void_p), ("normals", C.c_void_p), ("colors", C.c_void_p), ("features", C.c_void_p),
                ("F", C.c_int32), ("n_bound", C.c_int64), ("n_dev", C.c_void_p),
                ("points_out", C.c_void_p), ("normals_out", C.c_void_p), ("colors_out", C.c_void_p),
                ("features_out", C.c_void_p), ("capacity_out", C.c_int64), ("keep", C.c_void_p),
                ("marks", C.c_void_p), ("n_marks", C.c_int32), ("young_mark", C.c_int32),
                ("n_out", C.c_void_p), ("removed_out", C.c_void_p), ("scratch", C.c_void_p)]


class CarveSeq(C.Structure):
    """gs_carve_seq: one map, its L depth views with poses, and the two outputs of gs_free_space_dc_f32."""
    _fields_ = [("map", MapView), ("depth", C.c_void_p), ("depth_stride_view", C.c_int64), ("poses16", C.c_void_p),
                ("K16", C.c_void_p), ("violations", C.c_void_p), ("keep", C.c_void_p)]


class VoxelKeepSeq(C.Structure):
    """gs_voxel_keep_seq: one map's points and confidences, the outputs and the table scratch of gs_voxel_keep_dc_f32."""
    _fields_ = [("points", C.c_void_p), ("confidence", C.c_void_p), ("n_bound", C.c_int64), ("n_dev", C.c_void_p),
                ("keep", C.c_void_p), ("winner", C.c_void_p), ("unplaced", C.c_void_p), ("scratch", C.c_void_p),
                ("scratch_bytes", C.c_int64)]


class PicpSeq(C.Structure):
    """gs_picp_seq: one live frame, the model view's index image and the map for the projective ICP."""
    _fields_ = [("vertex", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("K16", C.c_void_p),
                ("index", C.c_void_p), ("model_pose16", C.c_void_p), ("map", MapView), ("init_pose16", C.c_void_p),
                ("out_pose16", C.c_void_p), ("trace", C.c_void_p), ("scratch", C.c_void_p)]


class PicpBackwardSeq(C.Structure):
    """gs_picp_backward_seq: the forward's inputs, its tape, the upstream adjoint and the gradient outputs."""
    _fields_ = [("vertex", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("K16", C.c_void_p),
                ("index", C.c_void_p), ("model_pose16", C.c_void_p), ("map", MapView), ("tape", C.c_void_p),
                ("pose_bar16", C.c_void_p), ("vertex_bar", C.c_void_p), ("points_bar", C.c_void_p),
                ("normals_bar", C.c_void_p), ("init_pose_bar16", C.c_void_p), ("scratch", C.c_void_p),
                ("scratch_bytes", C.c_int64)]


class PicpOrderedBackwardSeq(C.Structure):
    """gs_picp_ordered_backward_seq: gs_picp_backward_seq plus the optional copies of the record (keys, contributions)."""
    _fields_ = [("base", PicpBackwardSeq), ("key_out", C.c_void_p), ("contrib_out", C.c_void_p)]


class PicpColorSeq(C.Structure):
    """gs_picp_color_seq: gs_picp_seq plus the live colour image and the model intensity of the view."""
    _fields_ = [("base", PicpSeq), ("color", C.c_void_p), ("model_intensity", C.c_void_p)]


class FeatureFuseSeq(C.Structure):
    """gs_feature_fuse_seq: one sequence's feature layer, the tables of its frame and the outputs of the fusion."""
    _fields_ = [("emb", C.c_void_p), ("weight", C.c_void_p), ("capacity", C.c_int64), ("n_old_bound", C.c_int64),
                ("n_old_dev", C.c_void_p), ("best_pix", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p),
                ("feat", C.c_void_p), ("valid", C.c_void_p), ("row_of_pix", C.c_void_p), ("n_out", C.c_void_p),
                ("scratch", C.c_void_p)]


class FeatureCompactSeq(C.Structure):
    """gs_feature_compact_seq: one sequence's feature layer, its keep mask and the destination buffers."""
    _fields_ = [("emb", C.c_void_p), ("weight", C.c_void_p), ("n_bound", C.c_int64), ("n_dev", C.c_void_p),
                ("keep", C.c_void_p), ("emb_out", C.c_void_p), ("weight_out", C.c_void_p), ("capacity_out", C.c_int64),
                ("n_out", C.c_void_p), ("scratch", C.c_void_p)]


FEATURE_F32, FEATURE_F16 = 0, 1


class PicpParams(C.Structure):
    _fields_ = [("stride", C.c_int), ("numiters", C.c_int), ("damp", C.c_float), ("dist_th", C.c_float),
                ("dot_th", C.c_float)]


# name -> argtypes (return type is int unless listed in _RESTYPE)
_PROTOS = {
    "gs_abi_version": [],
    "gs_last_error": [],
    "gs_scratch_bytes": [_i64, _i64],
    "gs_profile_begin": [_i32],
    "gs_profile_end": [],
    "gs_profile_read": [_i32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)],
    "gs_frame_maps_f32": [_vp, _vp, _i32, _i32, _f, _vp, _vp, _vp, _vp, _vp],
    "gs_global_maps_f32": [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "gs_alpha_f32": [_vp, _i64, _f, _f, _vp, _vp],
    "gs_alpha_backward_f32": [_vp, _i64, _f, _f, _vp, _vp, _vp, _vp],
    "gs_downsample_frame_f32": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_project_map_f32": [_vp, _i64, _vp, _vp, _i32, _i32, _vp, _vp],
    "gs_active_table_i64": [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp],
    "gs_select_targets_f32": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "gs_downsample_table_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_knn1_f32": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp],
    "gs_knn1_grid_scratch_bytes": [_i64, _i64],
    "gs_knn1_grid_f32": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, C.POINTER(C.c_int64), _vp],
    "gs_gauss_newton_rows_f32": [_vp, _i64, _vp, _vp, _i64, _f, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_solve_normal_eq_f32": [_vp, _vp, _vp, _i64, _i32, _f, _vp, _vp],
    "gs_se3_exp_f32": [_vp, _vp, _vp],
    "gs_se3_exp_backward_f32": [_vp, _vp, _vp, _vp],
    "gs_transform_points_f32": [_vp, _i64, _vp, _vp, _vp],
    "gs_icp_scratch_bytes": [_i64, _i64],
    "gs_icp_f32": [_vp, _i64, _vp, _vp, _i64, _vp, _vp, C.POINTER(IcpParams), _vp, _vp, _vp, _vp],
    "gs_icp_trace_f32": [_vp, _i32, _vp, _vp],
    "gs_icp_dc_f32": [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, C.POINTER(IcpParams), _vp, _vp, _vp, _vp],
    "gs_frame_maps_backward_f32": [_vp, _vp, _i32, _i32, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_frame_maps_backward_kbar_scratch_bytes": [_i32, _i32],
    "gs_global_maps_backward_f32": [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "gs_downsample_frame_backward_f32": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "gs_icp_tape_bytes": [_i64, _i32],
    "gs_icp_tape_f32": [_vp, _i64, _vp, _vp, _i64, _vp, _vp, C.POINTER(IcpParams), _vp, _vp, _vp, _vp, _vp],
    "gs_icp_backward_scratch_bytes": [_i64, _i64],
    "gs_icp_backward_f32": [_vp, _vp, _i64, _vp, _vp, _i64, _vp, C.POINTER(IcpParams), _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp],
    "gs_similar_rows_f32": [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _f, _f, _vp, _vp],
    "gs_best_unique_rows_f32": [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp],
    "gs_associate_f32": [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f, _f, _vp, _vp, _vp, _vp],
    "gs_best_table_i64": [_vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp],
    "gs_rows_to_best_pix": [_vp, _i64, _i32, _i32, _vp, _vp],
    "gs_fuse_append_f32": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                           _vp, _vp, _vp],
    "gs_append_valid_f32": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "gs_ingest_depth_u16_f32": [_vp, _i32, _i32, _vp, _i32, _i32, C.c_double, _vp],
    "gs_ingest_color_u8_f32": [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp],
    "gs_ingest_frames_native_f32": [_vp, _vp, _i64, _i32, _i32, C.c_double, _i32, _vp, _vp, _vp],
    "gs_host_device_pointer": [_vp, C.POINTER(C.c_void_p)],
    "gs_global_maps_pose_backward_scratch_bytes": [_i32, _i32],
    "gs_global_maps_pose_backward_f32": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "gs_fuse_append_backward_f32": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp,
                                    _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_update_map_scratch_bytes": [_i64, _i32, _i32],
    "gs_update_map_fusion_dc_f32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32,
                                    _f, _f, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_icp_map_dc_f32": [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _vp, _vp, C.POINTER(IcpParams), _vp, _vp,
                          _vp],
    "gs_lattice_source_f32": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp],
    "gs_relative_pose_f32": [_vp, _vp, _i64, _vp, _vp],
    "gs_project_map_dc_f32": [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "gs_select_targets_dc_f32": [_vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "gs_associate_dc_f32": [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f, _f, _vp, _vp, _vp, _vp],
    "gs_fuse_append_dc_f32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                              _vp, _vp, _vp],
    "gs_append_valid_dc_f32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp,
                               _vp],
    "gs_frame_maps_batch_f32": [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _f, _vp, _vp, _vp, _vp],
    "gs_localize_scratch_bytes": [_i32, _i32, _i32, _i64],
    "gs_localize_batch_f32": [C.POINTER(LocalizeSeq), _i32, _i32, _i32, _i32, C.POINTER(IcpParams), _vp],
    "gs_update_map_fusion_batch_f32": [C.POINTER(UpdateSeq), _i32, _i32, _i32, _f, _f, _i32, _vp],
    "gs_project_points_f32": [_vp, _i32, _i64, _vp, _i64, _vp, _vp],
    "gs_unproject_points_f32": [_vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp],
    "gs_lie_small_f32": [_i32, _vp, _vp, _vp],
    "gs_localize_list_stats_i64": [_vp, _i32, _i32, _i32, _i64, C.POINTER(C.c_int64), _vp],
    "gs_localize_solve_stats_i64": [_vp, _i32, _i32, _i32, _i64, C.POINTER(C.c_int64), _vp],
    "gs_pointfusion_step_batch_f32": [C.POINTER(StepSeq), _i32, _i32, _i32, _i32, C.POINTER(IcpParams), _f, _f, _f, _i32, _vp],
    "gs_render_scratch_bytes": [_i32, _i32, _i32],
    "gs_render_map_dc_f32": [C.POINTER(RenderSeq), _i32, _i32, _i32, _i32, _i32, _f, _i32, _vp],
    "gs_render_backward_scratch_bytes": [_i32, _i32, _i32, _i64],
    "gs_render_map_backward_dc_f32": [C.POINTER(RenderBackwardSeq), _i32, _i32, _i32, _i32, _i32, _vp],
    "gs_surfel_radius_f32": [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp],
    "gs_render_map_radii_dc_f32": [C.POINTER(RenderSeq), C.POINTER(C.c_void_p), _i32, _i32, _i32, _i32, _i32, _f, _i32,
                                   _vp],
    "gs_render_map_radii_backward_dc_f32": [C.POINTER(RenderBackwardSeq), C.POINTER(C.c_void_p), _i32, _i32, _i32, _i32,
                                            _i32, _vp],
    "gs_prune_scratch_bytes": [_i64],
    "gs_prune_map_dc_f32": [C.POINTER(PruneSeq), _i32, _f, _i32, _vp],
    "gs_free_space_dc_f32": [C.POINTER(CarveSeq), _i32, _i32, _i32, _i32, _f, _i32, _i32, _vp],
    "gs_voxel_keep_scratch_bytes": [_i64],
    "gs_voxel_keep_dc_f32": [C.POINTER(VoxelKeepSeq), _i32, _f, _vp],
    "gs_bilateral_depth_f32": [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _f, _f, _vp, _vp, _vp],
    "gs_bilateral_depth_backward_f32": [_vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f, _f, _vp, _vp],
    "gs_projective_icp_scratch_bytes": [_i32, _i32, _i32],
    "gs_projective_icp_batch_f32": [C.POINTER(PicpSeq), _i32, _i32, _i32, C.POINTER(PicpParams), _vp],
    "gs_projective_icp_rows_f32": [C.POINTER(PicpSeq), _i32, _i32, _i32, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_projective_icp_tape_bytes": [_i32],
    "gs_projective_icp_tape_batch_f32": [C.POINTER(PicpSeq), C.POINTER(C.c_void_p), _i32, _i32, _i32,
                                         C.POINTER(PicpParams), _vp],
    "gs_projective_icp_backward_scratch_bytes": [_i32, _i32, _i32, _i64],
    "gs_projective_icp_backward_batch_f32": [C.POINTER(PicpBackwardSeq), _i32, _i32, _i32, C.POINTER(PicpParams), _vp],
    "gs_projective_icp_ordered_backward_scratch_bytes": [_i32, _i32, _i32, _i64],
    "gs_projective_icp_ordered_backward_sort_scratch_bytes": [_i32, _i32, _i32, _i32],
    "gs_projective_icp_ordered_backward_batch_f32": [C.POINTER(PicpOrderedBackwardSeq), _i32, _i32, _i32,
                                                     C.POINTER(PicpParams), _f, _i32, _vp, _i64, _vp],
    "gs_model_intensity_f32": [_vp, _vp, _i32, _i32, _i32, _vp, _vp],
    "gs_projective_icp_color_scratch_bytes": [_i32, _i32, _i32],
    "gs_projective_icp_color_batch_f32": [C.POINTER(PicpColorSeq), _i32, _i32, _i32, C.POINTER(PicpParams), _f, _vp],
    "gs_projective_icp_color_rows_f32": [C.POINTER(PicpColorSeq), _i32, _i32, _i32, _f, _f, _f, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_projective_icp_robust_batch_f32": [C.POINTER(PicpSeq), C.POINTER(C.c_void_p), _i32, _i32, _i32,
                                           C.POINTER(PicpParams), _f, _vp],
    "gs_projective_icp_robust_rows_f32": [C.POINTER(PicpSeq), _i32, _i32, _i32, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp],
    "gs_projective_icp_robust_backward_batch_f32": [C.POINTER(PicpBackwardSeq), _i32, _i32, _i32, C.POINTER(PicpParams),
                                                    _f, _vp],
    "gs_projective_icp_color_robust_batch_f32": [C.POINTER(PicpColorSeq), _i32, _i32, _i32, C.POINTER(PicpParams), _f, _f,
                                                 _f, _vp],
    "gs_projective_icp_color_robust_rows_f32": [C.POINTER(PicpColorSeq), _i32, _i32, _i32, _f, _f, _f, _f, _f, _vp, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_projective_icp_scaled_scratch_bytes": [_i32, _i32, _i32],
    "gs_projective_icp_color_scaled_scratch_bytes": [_i32, _i32, _i32],
    "gs_projective_icp_scaled_batch_f32": [C.POINTER(PicpSeq), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _i32, _i32,
                                           _i32, C.POINTER(PicpParams), _f, _f, _vp],
    "gs_projective_icp_scaled_rows_f32": [C.POINTER(PicpSeq), _i32, _i32, _i32, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp],
    "gs_projective_icp_color_scaled_batch_f32": [C.POINTER(PicpColorSeq), C.POINTER(C.c_void_p), _i32, _i32, _i32,
                                                 C.POINTER(PicpParams), _f, _f, _f, _f, _vp],
    "gs_projective_icp_scaled_backward_batch_f32": [C.POINTER(PicpBackwardSeq), _i32, _i32, _i32, C.POINTER(PicpParams),
                                                    _vp],
    "gs_projective_icp_color_joint_scaled_scratch_bytes": [_i32, _i32, _i32],
    "gs_projective_icp_color_joint_scaled_batch_f32": [C.POINTER(PicpColorSeq), C.POINTER(C.c_void_p),
                                                       C.POINTER(C.c_void_p), _i32, _i32, _i32, C.POINTER(PicpParams),
                                                       _f, _f, _f, _f, _f, _vp],
    "gs_projective_icp_color_joint_scaled_rows_f32": [C.POINTER(PicpColorSeq), _i32, _i32, _i32, _f, _f, _f, _f, _f, _f,
                                                      _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                      _vp, _vp, _vp],
    "gs_projective_icp_weighted_batch_f32": [C.POINTER(PicpSeq), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), _i32, _i32, _i32, C.POINTER(PicpParams), _f, _f, _vp],
    "gs_projective_icp_weighted_rows_f32": [C.POINTER(PicpSeq), _vp, _i32, _i32, _i32, _f, _f, _f, _f, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _vp],
    "gs_projective_icp_color_weighted_batch_f32": [C.POINTER(PicpColorSeq), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                   C.POINTER(C.c_void_p), _i32, _i32, _i32, C.POINTER(PicpParams), _f, _f,
                                                   _f, _f, _f, _vp],
    "gs_projective_icp_color_weighted_rows_f32": [C.POINTER(PicpColorSeq), _vp, _i32, _i32, _i32, _f, _f, _f, _f, _f, _f,
                                                  _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp],
    "gs_projective_icp_weighted_backward_scratch_bytes": [_i32, _i32, _i32, _i64, _i32],
    "gs_projective_icp_weighted_backward_batch_f32": [C.POINTER(PicpOrderedBackwardSeq), C.POINTER(C.c_void_p),
                                                      C.POINTER(C.c_void_p), _i32, _i32, _i32, C.POINTER(PicpParams),
                                                      _f, _i32, _i32, _vp, _i64, _vp],
    "gs_picp_outlier_classes_scratch_bytes": [_i32, _i32],
    "gs_picp_outlier_classes_batch_f32": [C.POINTER(PicpSeq), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), _i32, _i32, _i32, _f, _f, _f, _f, _f, _vp],
    "gs_region_mask_u8": [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _f, _vp],
    "gs_fuse_features_batch": [C.POINTER(FeatureFuseSeq), _i32, _i32, _i32, _i32, _i32, _vp],
    "gs_compact_features_batch": [C.POINTER(FeatureCompactSeq), _i32, _i32, _i32, _vp],
}
_RESTYPE = {"gs_last_error": C.c_char_p, "gs_scratch_bytes": _i64, "gs_icp_scratch_bytes": _i64,
            "gs_knn1_grid_scratch_bytes": _i64, "gs_update_map_scratch_bytes": _i64, "gs_global_maps_pose_backward_scratch_bytes": _i64, "gs_icp_tape_bytes": _i64, "gs_icp_backward_scratch_bytes": _i64,
            "gs_localize_scratch_bytes": _i64, "gs_frame_maps_backward_kbar_scratch_bytes": _i64,
            "gs_render_scratch_bytes": _i64, "gs_render_backward_scratch_bytes": _i64,
            "gs_prune_scratch_bytes": _i64, "gs_projective_icp_scratch_bytes": _i64,
            "gs_projective_icp_tape_bytes": _i64, "gs_projective_icp_backward_scratch_bytes": _i64,
            "gs_projective_icp_color_scratch_bytes": _i64, "gs_projective_icp_scaled_scratch_bytes": _i64,
            "gs_projective_icp_color_scaled_scratch_bytes": _i64,
            "gs_projective_icp_color_joint_scaled_scratch_bytes": _i64, "gs_voxel_keep_scratch_bytes": _i64,
            "gs_projective_icp_ordered_backward_scratch_bytes": _i64,
            "gs_projective_icp_ordered_backward_sort_scratch_bytes": _i64,
            "gs_projective_icp_weighted_backward_scratch_bytes": _i64,
            "gs_picp_outlier_classes_scratch_bytes": _i64}
EXPORTS = tuple(_PROTOS)


class HipExtensionError(RuntimeError):
    pass


def lib():
    """Loads libgradslam_hip.so (once).  Fails loudly: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionError(
                "gradslam_amd: %s is missing. Build it with `python -m gradslam_amd.csrc.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU / PyTorch fallback." % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            fn = getattr(handle, name)  # AttributeError if the .so does not export it
            fn.argtypes = argtypes
            fn.restype = _RESTYPE.get(name, C.c_int)
        if handle.gs_abi_version() != ABI_VERSION:
            raise HipExtensionError("libgradslam_hip.so ABI %d != expected %d; rebuild"
                                    % (handle.gs_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        raise HipExtensionError("%s failed (code %d): %s" % (what, status, lib().gs_last_error().decode()))


def require_device(*tensors):
    """Every tensor handed to the HIP library must be a contiguous tensor on a HIP device."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HipExtensionError(
                "gradslam_amd kernels run on the GPU only (got a %s tensor). Move the data to a HIP "
                "device; there is no CPU fallback." % t.device)
        if not t.is_contiguous():
            raise HipExtensionError("internal error: non-contiguous tensor passed to the HIP library")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise HipExtensionError("tensors live on different devices: %s vs %s" % (dev, t.device))
    return dev


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """Scratch buffers per (device, stream), grown on demand and reused every frame (the library never allocates).
    Keyed by the stream the calls are enqueued on: two chains of calls on different streams never share scratch."""
    _instances = {}

    def __init__(self, device):
        self.device = device
        self._bufs = {}

    @classmethod
    def get(cls, device):
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        ws = cls._instances.get(key)
        if ws is None:
            ws = cls._instances[key] = Workspace(device)
        return ws

    def bytes(self, name, nbytes):
        buf = self._bufs.get(name)
        if buf is None or buf.numel() < nbytes:
            nbytes = int(nbytes * 1.5) + 4096
            buf = self._bufs[name] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return buf

    def scratch(self, n_map, n_pix):
        return self.bytes("scratch", lib().gs_scratch_bytes(int(n_map), int(n_pix)))

    def tensor(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= int(s)
        item = torch.empty((), dtype=dtype).element_size()
        buf = self.bytes(name, max(n, 1) * item)
        return buf[: n * item].view(dtype).view(*shape)
