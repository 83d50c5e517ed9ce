"""ctypes binding of liblvba_hip.so (include/lvba_hip.h).  No torch types cross this boundary."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LVBA_HIP_LIB") or os.path.join(HERE, "liblvba_hip.so")  # override: A/B runs of two builds

# every extern "C" symbol include/lvba_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "lvba_version", "lvba_last_error", "lvba_device_count", "lvba_balm_default_opts", "lvba_shard_range",
    "lvba_balm_create", "lvba_balm_create_dev", "lvba_balm_destroy", "lvba_balm_configure", "lvba_balm_info", "lvba_balm_cost",
    "lvba_balm_eval", "lvba_balm_eval_blocks", "lvba_balm_solve", "lvba_balm_refine", "lvba_balm_lm_begin", "lvba_balm_lm_step",
    "lvba_balm_lm_end", "lvba_balm_set_groups", "lvba_balm_refine_groups", "lvba_balm_set_profiling", "lvba_balm_get_profile", "lvba_balm_get_ordering", "lvba_balm_nd_model", "lvba_balm_pair_layout", "lvba_balm_eval_layout",
    "lvba_balm_set_priors", "lvba_balm_prior_residuals", "lvba_cov_default_opts", "lvba_balm_covariance",
    "lvba_balm_set_loss", "lvba_balm_voxel_residuals",
    "lvba_dist_unique_id", "lvba_balm_dist_init", "lvba_balm_dist_init_external", "lvba_visual_dist_init_external",
    "lvba_visual_default_opts", "lvba_visual_create", "lvba_visual_destroy", "lvba_visual_cost", "lvba_visual_linearize", "lvba_visual_solve", "lvba_visual_info", "lvba_visual_pair_layout", "lvba_visual_eval_layout", "lvba_visual_dist_init",
    "lvba_visual_refine", "lvba_visual_set_loss", "lvba_visual_residual_sq", "lvba_visual_set_priors", "lvba_visual_prior_residuals",
    "lvba_voxel_default_opts", "lvba_voxmap_build", "lvba_voxmap_destroy", "lvba_voxmap_info", "lvba_voxmap_export",
    "lvba_voxmap_to_balm", "lvba_voxmap_find_planes", "lvba_scans_create", "lvba_scans_destroy", "lvba_voxmap_build_scans",
    "lvba_release_cached_memory", "lvba_window_default_opts", "lvba_window_ba", "lvba_window_split", "lvba_window_ba_multi", "lvba_scans_info", "lvba_scans_download",
    "lvba_lidar_ba_default_opts", "lvba_lidar_ba", "lvba_lidar_ba_multi", "lvba_lidar_ba_priors", "lvba_lidar_ba_multi_priors", "lvba_lidar_ba_robust", "lvba_triangulate_tracks",
    "lvba_depth_render", "lvba_depth_upload", "lvba_depth_info", "lvba_depth_download", "lvba_depth_destroy",
    "lvba_fuse_default_opts", "lvba_fuse_tracks",
    "lvba_colorize_default_opts", "lvba_colorize_create", "lvba_colorize_add_images", "lvba_colorize_count",
    "lvba_colorize_download", "lvba_colorize_profile", "lvba_colorize_destroy",
    "lvba_mapq_default_opts", "lvba_mapq_scans", "lvba_mapq_points",
    "lvba_dynamic_default_opts", "lvba_dynamic_labels", "lvba_scans_select",
    "lvba_register_default_opts", "lvba_register_linearize", "lvba_register_scans",
    "lvba_submaps_build", "lvba_submaps_count", "lvba_submaps_find_planes", "lvba_register_linearize_submaps",
    "lvba_register_scans_submaps", "lvba_loop_default_opts", "lvba_loop_candidates",
    "lvba_place_default_opts", "lvba_place_descriptors", "lvba_place_search", "lvba_place_candidates",
    "lvba_closure_default_opts", "lvba_closure_consistency",
    "lvba_posegraph_default_opts", "lvba_posegraph_relax",
    "lvba_match_default_opts", "lvba_match_create", "lvba_match_destroy", "lvba_match_set_geometry", "lvba_match_pairs",
    "lvba_match_scan", "lvba_match_set_depth", "lvba_match_points",
    "lvba_covis_default_opts", "lvba_covis_samples", "lvba_covis_counts", "lvba_covis_pairs",
    "lvba_trackgraph_create", "lvba_trackgraph_components", "lvba_trackgraph_orders", "lvba_trackgraph_destroy",
    "lvba_verify_default_opts", "lvba_verify_create", "lvba_verify_destroy", "lvba_verify_pairs", "lvba_verify_hypotheses",
    "lvba_verify_score", "lvba_verify_pairs_model", "lvba_verify_hypotheses_homography", "lvba_verify_score_homography",
    "lvba_sift_default_opts", "lvba_sift_tile_width", "lvba_sift_blur_taps", "lvba_sift_extract", "lvba_sift_profile", "lvba_sift_pyramid",
    "lvba_sift_candidates",
    "lvba_resect_default_opts", "lvba_resect_images", "lvba_resect_hypotheses", "lvba_resect_score", "lvba_resect_lift",
    "lvba_calib_default_opts", "lvba_calib_extrinsic", "lvba_calib_linearize",
    "lvba_calib_td_default_opts", "lvba_calib_extrinsic_td", "lvba_calib_linearize_td",
    "lvba_photo_default_opts", "lvba_photo_create", "lvba_photo_add_images", "lvba_photo_finish", "lvba_photo_sums", "lvba_photo_free",
    "lvba_palign_default_opts", "lvba_palign_create", "lvba_palign_linearize", "lvba_palign_align", "lvba_palign_profile", "lvba_palign_free",
    "lvba_expo_default_opts", "lvba_expo_create", "lvba_expo_sums", "lvba_expo_solve", "lvba_expo_profile", "lvba_expo_free",
    "lvba_photo_add_images_gains",
    "lvba_undistort_default_opts", "lvba_undistort_tile", "lvba_undistort_create", "lvba_undistort_info", "lvba_undistort_images",
    "lvba_undistort_map", "lvba_undistort_profile", "lvba_undistort_free",
]

OK, ERR_ARG, ERR_DEVICE, ERR_NOMEM, ERR_UNSUPPORTED, ERR_DIST, ERR_STATE = 0, -1, -2, -3, -4, -5, -6
NUM_FACTORIZATION, NUM_NONFINITE = 1, 2
PADDING = ("reserved", "pad")     # field names of the header that carry nothing


class Struct(C.Structure):
    """The base of every mirror below: as_dict() is the struct's fields by name, arrays as lists."""
    _hidden = ()                  # fields as_dict leaves out

    def as_dict(self):
        out = {}
        for f, _ in self._fields_:
            if f not in self._hidden:
                v = getattr(self, f)
                out[f] = list(v) if isinstance(v, C.Array) else v
        return out


class CovOpts(Struct):
    _fields_ = [("anchor", C.c_int32), ("reserved", C.c_int32), ("min_pivot_ratio", C.c_double)]


class BalmOpts(Struct):
    _fields_ = [("max_iter", C.c_int32), ("reserved", C.c_int32), ("u0", C.c_double), ("v0", C.c_double),
                ("rel_tol", C.c_double)]


class LmTrace(Struct):
    _fields_ = [("iter", C.c_int32), ("accepted", C.c_int32), ("evaluated", C.c_int32), ("status", C.c_int32),
                ("residual1", C.c_double), ("residual2", C.c_double), ("u", C.c_double), ("v", C.c_double),
                ("q", C.c_double), ("q1", C.c_double)]


class BalmInfo(Struct):
    _fields_ = [("n_poses", C.c_int32), ("n_ranks", C.c_int32), ("n_voxels", C.c_int64),
                ("n_voxels_global", C.c_int64), ("n_factors", C.c_int64), ("n_pairs", C.c_int64),
                ("n_chunks", C.c_int64), ("n_blocks", C.c_int64), ("band_blocks", C.c_int32), ("use_band", C.c_int32),
                ("hess_bytes", C.c_int64), ("device_bytes", C.c_int64), ("allreduce_bytes", C.c_int64),
                ("twist_panels", C.c_int32), ("solve_ranks", C.c_int32), ("trial_linearised", C.c_int32), ("y_fp32", C.c_int32),
                ("nd_kind", C.c_int32), ("nd_arcs", C.c_int32), ("nd_sep_poses", C.c_int32), ("nd_sep_band_blocks", C.c_int32),
                ("nd_model_band_ms", C.c_double), ("nd_model_nd_ms", C.c_double)]


class PairLayout(Struct):
    _fields_ = [("form", C.c_int32), ("cut", C.c_int32), ("n_items", C.c_int64), ("n_multi", C.c_int64), ("n_partial", C.c_int64),
                ("window_voxels", C.c_int64), ("longest_item", C.c_int64), ("longest_multi", C.c_int64)]


def pair_layout(fn, handle):
    """lvba_balm_pair_layout / lvba_visual_pair_layout: the struct's fields plus item_len / item_slot [n_items] (int64)."""
    o = PairLayout()
    check(fn(handle, C.byref(o), None, None, 0))
    n = int(o.n_items)
    item_len, item_slot = np.zeros(n, np.int64), np.zeros(n, np.int64)
    if n:
        check(fn(handle, C.byref(o), item_len.ctypes.data, item_slot.ctypes.data, n))
    d = o.as_dict()
    d["item_len"], d["item_slot"] = item_len, item_slot
    return d


class EvalLayout(Struct):
    _fields_ = [("slices", C.c_int32), ("unit_form", C.c_int32), ("units", C.c_int64), ("unit_grid", C.c_int64),
                ("point_groups", C.c_int32), ("back_groups", C.c_int32), ("point_grid", C.c_int64), ("back_grid", C.c_int64),
                ("n_groups", C.c_int64), ("n_factors", C.c_int64), ("n_chunks", C.c_int64)]


def eval_layout(fn, handle):
    """lvba_balm_eval_layout / lvba_visual_eval_layout: the struct's fields."""
    o = EvalLayout()
    check(fn(handle, C.byref(o)))
    return o.as_dict()


class NdModel(Struct):
    _fields_ = [("n_ranks", C.c_int32), ("arcs", C.c_int32), ("sep_poses", C.c_int32), ("sep_band_blocks", C.c_int32),
                ("max_arc_poses", C.c_int32), ("max_arc_band_blocks", C.c_int32), ("band_ms", C.c_double), ("nd_ms", C.c_double)]


class Prof(Struct):
    _fields_ = [("cost_ms", C.c_double), ("cost_calls", C.c_int64), ("eval_ms", C.c_double),
                ("eval_calls", C.c_int64), ("solve_ms", C.c_double), ("solve_calls", C.c_int64),
                ("reduce_ms", C.c_double), ("reduce_calls", C.c_int64), ("cost_kernel_ms", C.c_double),
                ("eval_kernel_ms", C.c_double)]


class VisualOpts(Struct):
    _fields_ = [("max_iter", C.c_int32), ("reserved", C.c_int32), ("initial_radius", C.c_double), ("max_radius", C.c_double),
                ("min_radius", C.c_double), ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double)]


class VisualTrace(Struct):
    _fields_ = [("iter", C.c_int32), ("accepted", C.c_int32), ("valid", C.c_int32), ("reserved", C.c_int32),
                ("cost", C.c_double), ("cost_change", C.c_double), ("step_norm", C.c_double), ("radius", C.c_double),
                ("rho", C.c_double), ("gradient_max_norm", C.c_double)]
    _hidden = PADDING


PRIOR_KINDS = {"pose": 0, "position": 1, "relative": 2}


class Prior(Struct):
    """lvba_prior: one pose prior (see balm.Prior for the constructors)"""
    _fields_ = [("kind", C.c_int32), ("i", C.c_int32), ("j", C.c_int32), ("reserved", C.c_int32), ("meas", C.c_double * 12),
                ("offset_i", C.c_double * 12), ("offset_j", C.c_double * 12), ("sqrt_info", C.c_double * 36)]


LOSS_KINDS = {"trivial": 0, "huber": 1, "softlone": 2, "cauchy": 3, "arctan": 4, "tukey": 5}


class Loss(Struct):
    """lvba_loss: kind (LVBA_LOSS_*), scale a (visual stage: whitened residual units; LiDAR stage: metres)."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_double)]


class PosegraphOpts(Struct):
    """lvba_posegraph_opts (include/lvba_hip.h)"""
    _fields_ = [("anchor", C.c_int32), ("max_iter", C.c_int32), ("odom_sigma_rot", C.c_double), ("odom_sigma_pos", C.c_double),
                ("anchor_sigma_rot", C.c_double), ("anchor_sigma_pos", C.c_double), ("rel_tol", C.c_double), ("closure_loss", Loss)]


class PosegraphReport(Struct):
    """lvba_posegraph_report"""
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("status", C.c_int32), ("solver_kind", C.c_int32),
                ("cost_first", C.c_double), ("cost_last", C.c_double), ("odom_cost_last", C.c_double),
                ("closure_cost_last", C.c_double), ("max_step_last", C.c_double)]


PG_SOLVER_KINDS = {-1: "none", 0: "band", 1: "dissected", 2: "dense"}


def loss_struct(loss):
    """None -> NULL (TRIVIAL); (kind, scale) -> a pointer to an lvba_loss.  Shared by VisualProblem.set_loss, BalmProblem.set_loss
    and the pipeline's LiDAR losses."""
    if loss is None:
        return None
    kind, scale = loss
    k = LOSS_KINDS.get(str(kind).lower()) if isinstance(kind, str) else int(kind)
    if k is None:
        raise ValueError(f"unknown loss kind {kind!r}; one of {sorted(LOSS_KINDS)}")
    return C.pointer(Loss(k, 0, float(scale)))


class FuseOpts(Struct):
    _fields_ = [("obser_thr", C.c_int32), ("reserved", C.c_int32), ("min_view_angle_deg", C.c_double),
                ("reproj_mean_thr_px", C.c_double)]


class ColorizeOpts(Struct):
    _fields_ = [("half_window_s", C.c_double), ("leaf_size", C.c_double), ("max_batch_images", C.c_int32),
                ("reserved", C.c_int32)]


class MapqOpts(Struct):
    _fields_ = [("radius", C.c_double), ("min_neighbors", C.c_int32), ("query_stride", C.c_int32)]


class MapqSummary(Struct):
    _fields_ = [("n_points", C.c_int64), ("n_queries", C.c_int64), ("n_valid", C.c_int64), ("mme", C.c_double), ("mpv", C.c_double),
                ("mean_neighbors", C.c_double), ("ms", C.c_double * 4)]


class DynamicOpts(Struct):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("halo", C.c_int32), ("window", C.c_int32), ("min_free", C.c_int32),
                ("batch_frames", C.c_int32), ("el_min", C.c_double), ("el_max", C.c_double), ("min_range", C.c_double),
                ("max_range", C.c_double), ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("free_ratio", C.c_double)]


class DynamicSummary(Struct):
    _fields_ = [("n_points", C.c_int64), ("n_judged", C.c_int64), ("n_dynamic", C.c_int64), ("ms", C.c_double * 4)]


REG_STATUS = {0: "converged", 1: "max_iterations", 2: "too_few_inliers", 3: "degenerate"}


class RegisterOpts(Struct):
    _fields_ = [("max_iterations", C.c_int32), ("max_distance", C.c_double), ("min_inliers", C.c_int64), ("min_eigenvalue", C.c_double),
                ("tol_rot", C.c_double), ("tol_pos", C.c_double), ("loss", Loss)]


class RegisterResult(Struct):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("inliers", C.c_int64), ("points", C.c_int64),
                ("cost_first", C.c_double), ("cost_last", C.c_double), ("rmse", C.c_double), ("min_eigenvalue", C.c_double)]


class LoopOpts(Struct):
    _fields_ = [("submap_size", C.c_int32), ("min_gap", C.c_int32), ("max_per_frame", C.c_int32), ("query_stride", C.c_int32),
                ("radius", C.c_double)]


class LoopCandidate(Struct):
    _fields_ = [("query", C.c_int32), ("submap", C.c_int32), ("ref", C.c_int32), ("pad", C.c_int32), ("distance", C.c_double)]


class PlaceOpts(Struct):
    _fields_ = [("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("min_range", C.c_double), ("max_range", C.c_double),
                ("z_offset", C.c_double), ("submap_size", C.c_int32), ("min_gap", C.c_int32), ("n_key_candidates", C.c_int32),
                ("max_per_frame", C.c_int32), ("query_stride", C.c_int32), ("pad", C.c_int32), ("max_distance", C.c_double)]


class PlaceCandidate(Struct):
    _fields_ = [("query", C.c_int32), ("submap", C.c_int32), ("ref", C.c_int32), ("shift", C.c_int32), ("distance", C.c_double),
                ("yaw", C.c_double)]


class ClosureOpts(Struct):
    _fields_ = [("rot_tol", C.c_double), ("rot_rate", C.c_double), ("trans_tol", C.c_double), ("trans_rate", C.c_double),
                ("n_seeds", C.c_int32), ("min_set", C.c_int32)]


class MatchOpts(Struct):
    """lvba_match_opts"""
    _fields_ = [("max_distance", C.c_double), ("max_ratio", C.c_double), ("mutual", C.c_int32), ("guided", C.c_int32),
                ("max_epipolar_px", C.c_double), ("max_reproj_px", C.c_double)]


class VerifyOpts(Struct):
    """lvba_verify_opts"""
    _fields_ = [("method", C.c_int32), ("hypotheses", C.c_int32), ("refine_rounds", C.c_int32), ("min_inliers", C.c_int32),
                ("max_error_px", C.c_double), ("seed", C.c_uint64)]


class ResectOpts(Struct):
    """lvba_resect_opts"""
    _fields_ = [("hypotheses", C.c_int32), ("refine_rounds", C.c_int32), ("min_inliers", C.c_int32), ("reserved", C.c_int32),
                ("max_error_px", C.c_double), ("seed", C.c_uint64)]


class CalibOpts(Struct):
    """lvba_calib_opts"""
    _fields_ = [("max_iterations", C.c_int32), ("loss_kind", C.c_int32), ("min_records", C.c_int64), ("loss_scale_px", C.c_double),
                ("max_error_px", C.c_double), ("min_eig_ratio", C.c_double), ("eps_rot", C.c_double), ("eps_trans", C.c_double),
                ("reserved", C.c_int64)]


class CalibTdOpts(Struct):
    """lvba_calib_td_opts"""
    _fields_ = [("calib", CalibOpts), ("eps_td_s", C.c_double), ("max_abs_td_s", C.c_double), ("reserved", C.c_int64)]


class PhotoOpts(Struct):
    """lvba_photo_opts"""
    _fields_ = [("occlusion_rel", C.c_double), ("occlusion_abs", C.c_double), ("max_depth", C.c_double), ("holes", C.c_int32),
                ("min_views", C.c_int32), ("max_batch_images", C.c_int32), ("reserved", C.c_int32)]


class PhotoSummary(Struct):
    """lvba_photo_summary"""
    _fields_ = [("n_points", C.c_int64), ("n_seen", C.c_int64), ("n_valid", C.c_int64), ("n_samples", C.c_int64),
                ("mean_sigma", C.c_double), ("mean_views", C.c_double), ("ms", C.c_double * 4)]


class PalignOpts(Struct):
    """lvba_palign_opts"""
    _fields_ = [("occlusion_rel", C.c_double), ("occlusion_abs", C.c_double), ("max_depth", C.c_double), ("loss_scale", C.c_double),
                ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("max_rotation_deg", C.c_double), ("max_translation", C.c_double),
                ("holes", C.c_int32), ("loss_kind", C.c_int32), ("min_samples", C.c_int32), ("max_iterations", C.c_int32),
                ("max_batch_images", C.c_int32), ("reserved", C.c_int32)]


class ExpoOpts(Struct):
    """lvba_expo_opts"""
    _fields_ = [("occlusion_rel", C.c_double), ("occlusion_abs", C.c_double), ("max_depth", C.c_double), ("min_gain", C.c_double),
                ("max_gain", C.c_double), ("max_offset", C.c_double), ("holes", C.c_int32), ("model", C.c_int32), ("sat_lo", C.c_int32),
                ("sat_hi", C.c_int32), ("gate", C.c_int32), ("min_samples", C.c_int32), ("min_spread", C.c_int32),
                ("max_batch_images", C.c_int32)]


class UndistortOpts(Struct):
    """lvba_undistort_opts"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("out_width", C.c_int32),
                ("out_height", C.c_int32), ("border", C.c_int32), ("max_batch_images", C.c_int32)]


class SiftOpts(Struct):
    """lvba_sift_opts"""
    _fields_ = [("first_octave", C.c_int32), ("n_intervals", C.c_int32), ("sigma0", C.c_double), ("dog_threshold", C.c_double),
                ("edge_threshold", C.c_double), ("orientation_window", C.c_double), ("max_orientations", C.c_int32),
                ("max_features", C.c_int32), ("chunk_images", C.c_int32), ("reserved", C.c_int32)]


class CovisOpts(Struct):
    """lvba_covis_opts"""
    _fields_ = [("grid_x", C.c_int32), ("grid_y", C.c_int32), ("search_radius", C.c_int32), ("occlusion", C.c_int32),
                ("both_ways", C.c_int32), ("max_per_image", C.c_int32), ("min_shared", C.c_int32), ("reserved", C.c_int32),
                ("min_overlap", C.c_double), ("occlusion_rel", C.c_double), ("occlusion_abs", C.c_double)]


class TrackGraphInfo(Struct):
    """lvba_trackgraph_info"""
    _fields_ = [("n_nodes", C.c_int64), ("n_edges", C.c_int64), ("n_skipped", C.c_int64), ("n_components_all", C.c_int64),
                ("n_components", C.c_int64), ("n_observations", C.c_int64), ("largest_component", C.c_int64),
                ("cc_rounds", C.c_int32), ("reserved", C.c_int32)]
    _hidden = PADDING


class VoxelOpts(Struct):
    _fields_ = [("voxel_size", C.c_double), ("eigen_ratio", C.c_float * 4), ("min_points", C.c_int32),
                ("layer_limit", C.c_int32)]


class VoxmapInfo(Struct):
    _fields_ = [("n_points", C.c_int64), ("n_roots", C.c_int64), ("n_planes", C.c_int64), ("n_voxels", C.c_int64),
                ("n_factors", C.c_int64), ("upload_ms", C.c_double), ("key_ms", C.c_double), ("sort_ms", C.c_double),
                ("count_ms", C.c_double), ("write_ms", C.c_double)]


class WindowOpts(Struct):
    _fields_ = [("window_size", C.c_int32), ("use_rel", C.c_int32), ("anchor_leaf", C.c_double), ("voxel", VoxelOpts),
                ("lm", BalmOpts), ("merge_only", C.c_int32), ("lm_mode", C.c_int32)]


class WindowInfo(Struct):
    _fields_ = [("start", C.c_int32), ("n_frames", C.c_int32), ("skipped", C.c_int32), ("anchor", C.c_int32),
                ("n_iter", C.c_int32), ("lm_status", C.c_int32), ("n_voxels", C.c_int64), ("n_factors", C.c_int64),
                ("n_anchor_points", C.c_int64), ("cost_first", C.c_double), ("cost_last", C.c_double), ("map_ms", C.c_double),
                ("solve_ms", C.c_double), ("merge_ms", C.c_double), ("setup_ms", C.c_double)]


class LidarBaOpts(Struct):
    _fields_ = [("window", WindowOpts), ("window_enable", C.c_int32), ("stage1_enable", C.c_int32),
                ("stage_voxel_size", C.c_double * 2), ("stage_eigen_ratio", (C.c_float * 4) * 2), ("lm", BalmOpts)]


class LidarBaReport(Struct):
    _fields_ = [("n_frames", C.c_int32), ("n_windows", C.c_int32), ("n_windows_skipped", C.c_int32), ("n_anchors", C.c_int32),
                ("stage_ran", C.c_int32 * 2), ("stage_iters", C.c_int32 * 2), ("stage_status", C.c_int32 * 2),
                ("reserved", C.c_int32), ("stage_voxels", C.c_int64 * 2), ("stage_factors", C.c_int64 * 2),
                ("stage_cost_first", C.c_double * 2), ("stage_cost_last", C.c_double * 2), ("window_ms", C.c_double),
                ("stage_ms", C.c_double * 2)]     # as_dict shows `reserved`, as it always has


TERMINATION = {0: "NO_CONVERGENCE", 1: "CONVERGENCE(function)", 2: "CONVERGENCE(parameter)", 3: "CONVERGENCE(gradient)",
               4: "CONVERGENCE(radius)", 5: "FAILURE"}


class LvbaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lvba status {code}: {msg}")
        self.code = code


# every struct typedef of include/lvba_hip.h and its mirror (tests/test_abi.py holds the two together field for field)
STRUCTS = {
    "lvba_balm_opts": BalmOpts, "lvba_lm_trace": LmTrace, "lvba_balm_info_t": BalmInfo, "lvba_prof_t": Prof,
    "lvba_pair_layout_t": PairLayout, "lvba_eval_layout_t": EvalLayout, "lvba_prior": Prior, "lvba_cov_opts": CovOpts,
    "lvba_loss": Loss, "lvba_nd_model_t": NdModel, "lvba_visual_opts": VisualOpts, "lvba_visual_trace": VisualTrace,
    "lvba_voxel_opts": VoxelOpts, "lvba_voxmap_info_t": VoxmapInfo, "lvba_fuse_opts": FuseOpts, "lvba_window_opts": WindowOpts,
    "lvba_window_info": WindowInfo, "lvba_lidar_ba_opts": LidarBaOpts, "lvba_lidar_ba_report": LidarBaReport,
    "lvba_colorize_opts": ColorizeOpts, "lvba_mapq_opts": MapqOpts, "lvba_mapq_summary": MapqSummary,
    "lvba_register_opts": RegisterOpts, "lvba_register_result": RegisterResult, "lvba_loop_opts": LoopOpts,
    "lvba_loop_candidate": LoopCandidate, "lvba_place_opts": PlaceOpts, "lvba_place_candidate": PlaceCandidate,
    "lvba_closure_opts": ClosureOpts, "lvba_posegraph_opts": PosegraphOpts, "lvba_posegraph_report": PosegraphReport,
    "lvba_match_opts": MatchOpts, "lvba_covis_opts": CovisOpts, "lvba_trackgraph_info": TrackGraphInfo,
    "lvba_verify_opts": VerifyOpts, "lvba_sift_opts": SiftOpts, "lvba_dynamic_opts": DynamicOpts,
    "lvba_dynamic_summary": DynamicSummary, "lvba_resect_opts": ResectOpts,
    "lvba_calib_opts": CalibOpts, "lvba_calib_td_opts": CalibTdOpts, "lvba_photo_opts": PhotoOpts, "lvba_photo_summary": PhotoSummary,
    "lvba_palign_opts": PalignOpts, "lvba_expo_opts": ExpoOpts, "lvba_undistort_opts": UndistortOpts,
}

_INTS = (C.c_int32, C.c_int64, C.c_uint64)
_FLOATS = (C.c_double, C.c_float)
_C_NAMES = {cls: name for name, cls in STRUCTS.items()}


def option_names(struct_cls):
    """The options of an opts struct that a keyword can set: its scalar fields in declaration order, without the padding.  Losses,
    arrays and nested structs are not keywords of make_opts; their module sets them on the result."""
    return tuple(f for f, t in struct_cls._fields_ if t in _INTS + _FLOATS and f not in PADDING)


def set_opts(o, what, _also=(), **kw):
    """Set the options `kw` in the opts struct o, each coerced to its field's type; TypeError on a name that is not an option.
    _also: the options the calling module sets itself, for the message."""
    names, types = option_names(type(o)), dict(o._fields_)
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"unknown {what} option {k!r}; one of {names + tuple(_also)}")
        setattr(o, k, float(v) if types[k] in _FLOATS else int(v))
    return o


def make_opts(struct_cls, what, _also=(), **kw):
    """A struct_cls with the library's defaults and `kw` over them: lvba_x_opts is filled by lvba_x_default_opts.  `what` names
    the kind of option in the error message."""
    o = struct_cls()
    lib_default_opts = getattr(load(), _C_NAMES[struct_cls][:-len("opts")] + "default_opts")
    lib_default_opts(C.byref(o))
    return set_opts(o, what, _also, **kw)


class Handle:
    """Owner of one library object: `_h` is its handle (None, 0 or an empty c_void_p: none), `lib` the loaded library, and
    `_destroy` names the symbol that frees it.  A context manager; close() may be called any number of times."""
    _destroy = None

    def close(self):
        h = getattr(self, "_h", None)          # absent when __init__ raised early
        if h is not None and getattr(h, "value", h):
            getattr(self.lib, self._destroy)(h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_lib = None


def load():
    """Load the HIP library.  Fails loudly if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the hot path)")
    lib = C.CDLL(LIB_PATH)
    f64p = np.ctypeslib.ndpointer(np.float64, flags="C")
    i64p = np.ctypeslib.ndpointer(np.int64, flags="C")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
    H = C.c_void_p
    lib.lvba_version.restype = C.c_int32
    lib.lvba_last_error.restype = C.c_char_p
    lib.lvba_device_count.restype = C.c_int32
    lib.lvba_balm_default_opts.argtypes = [C.POINTER(BalmOpts)]
    lib.lvba_shard_range.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.lvba_shard_range.restype = None
    lib.lvba_balm_create.argtypes = [C.c_int32, C.c_int64, i64p, i32p, f64p, C.c_int32, C.POINTER(H)]
    lib.lvba_balm_create_dev.argtypes = [C.c_int32, C.c_int64, i64p, i32p, C.c_void_p, C.c_int32, C.POINTER(H)]
    lib.lvba_balm_destroy.argtypes = [H]
    lib.lvba_balm_configure.argtypes = [H, C.c_int32, C.c_double]
    lib.lvba_balm_info.argtypes = [H, C.POINTER(BalmInfo)]
    lib.lvba_balm_cost.argtypes = [H, f64p, C.c_int32, C.POINTER(C.c_double)]
    lib.lvba_balm_eval.argtypes = [H, f64p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    lib.lvba_balm_eval_blocks.argtypes = [H, f64p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
                                          C.POINTER(C.c_double)]
    lib.lvba_balm_solve.argtypes = [H, C.c_double, f64p]
    lib.lvba_balm_refine.argtypes = [H, f64p, C.POINTER(BalmOpts), C.POINTER(LmTrace), C.POINTER(C.c_int32)]
    lib.lvba_balm_lm_begin.argtypes = [H, f64p, C.POINTER(BalmOpts)]
    lib.lvba_balm_lm_step.argtypes = [H, C.POINTER(LmTrace), C.POINTER(C.c_int32)]
    lib.lvba_balm_lm_end.argtypes = [H, C.c_void_p]
    lib.lvba_balm_set_groups.argtypes = [H, C.c_int32, i32p, i64p]
    lib.lvba_balm_refine_groups.argtypes = [H, f64p, C.POINTER(BalmOpts), i32p, i32p, f64p, f64p]
    lib.lvba_balm_set_profiling.argtypes = [H, C.c_int32]
    lib.lvba_balm_get_profile.argtypes = [H, C.POINTER(Prof), C.c_int32]
    lib.lvba_balm_get_ordering.argtypes = [H, i32p]
    lib.lvba_balm_nd_model.argtypes = [H, C.c_int32, C.POINTER(NdModel)]
    lib.lvba_balm_pair_layout.argtypes = [H, C.POINTER(PairLayout), C.c_void_p, C.c_void_p, C.c_int64]
    lib.lvba_visual_pair_layout.argtypes = [H, C.POINTER(PairLayout), C.c_void_p, C.c_void_p, C.c_int64]
    lib.lvba_balm_eval_layout.argtypes = [H, C.POINTER(EvalLayout)]
    lib.lvba_visual_eval_layout.argtypes = [H, C.POINTER(EvalLayout)]
    lib.lvba_balm_set_priors.argtypes = [H, C.c_int32, C.c_void_p]
    lib.lvba_balm_prior_residuals.argtypes = [H, f64p, C.c_void_p, C.POINTER(C.c_double)]
    lib.lvba_cov_default_opts.argtypes = [C.POINTER(CovOpts)]
    lib.lvba_balm_covariance.argtypes = [H, f64p, C.POINTER(CovOpts), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    lib.lvba_balm_set_loss.argtypes = [H, C.POINTER(Loss)]
    lib.lvba_balm_voxel_residuals.argtypes = [H, f64p, C.c_void_p, C.c_void_p]
    lib.lvba_dist_unique_id.argtypes = [C.c_char_p]
    lib.lvba_balm_dist_init_external.argtypes = [H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lvba_visual_dist_init_external.argtypes = [H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lvba_balm_dist_init.argtypes = [H, C.c_int32, C.c_int32, C.c_char_p]
    u8p = np.ctypeslib.ndpointer(np.uint8, flags="C")
    lib.lvba_visual_default_opts.argtypes = [C.POINTER(VisualOpts)]
    lib.lvba_visual_create.argtypes = [C.c_int32, C.c_int64, i64p, C.c_void_p, C.c_void_p, f64p, u8p, f64p, C.c_double,
                                       C.c_double, C.c_int32, C.POINTER(H)]
    lib.lvba_visual_destroy.argtypes = [H]
    lib.lvba_visual_cost.argtypes = [H, f64p, f64p, f64p, C.POINTER(C.c_double)]
    lib.lvba_visual_info.argtypes = [H, C.POINTER(BalmInfo)]
    lib.lvba_visual_dist_init.argtypes = [H, C.c_int32, C.c_int32, C.c_char_p]
    lib.lvba_visual_linearize.argtypes = [H, f64p, f64p, f64p, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    lib.lvba_visual_solve.argtypes = [H, f64p, C.POINTER(C.c_int32)]
    lib.lvba_visual_refine.argtypes = [H, f64p, f64p, f64p, C.POINTER(VisualOpts), C.POINTER(VisualTrace), C.c_int32,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lvba_visual_set_loss.argtypes = [H, C.POINTER(Loss), C.POINTER(Loss)]
    lib.lvba_visual_residual_sq.argtypes = [H, f64p, f64p, f64p, C.c_void_p, C.c_void_p]
    lib.lvba_visual_set_priors.argtypes = [H, C.c_int32, C.c_void_p]
    lib.lvba_visual_prior_residuals.argtypes = [H, f64p, f64p, C.c_void_p, C.POINTER(C.c_double)]
    lib.lvba_voxel_default_opts.argtypes = [C.POINTER(VoxelOpts)]
    lib.lvba_voxmap_build.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), i64p, C.c_int32, f64p,
                                      C.POINTER(VoxelOpts), C.POINTER(H)]
    lib.lvba_voxmap_destroy.argtypes = [H]
    lib.lvba_scans_create.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), i64p, C.c_int32, C.POINTER(H)]
    lib.lvba_scans_destroy.argtypes = [H]
    lib.lvba_voxmap_build_scans.argtypes = [H, C.c_int32, C.c_int32, f64p, C.POINTER(VoxelOpts), C.POINTER(H)]
    lib.lvba_voxmap_info.argtypes = [H, C.POINTER(VoxmapInfo)]
    lib.lvba_voxmap_export.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_voxmap_to_balm.argtypes = [H, C.POINTER(H)]
    lib.lvba_voxmap_find_planes.argtypes = [H, C.c_int64, f64p, f64p, u8p]
    lib.lvba_release_cached_memory.restype = C.c_int64
    lib.lvba_window_default_opts.argtypes = [C.POINTER(WindowOpts)]
    lib.lvba_window_ba.argtypes = [H, f64p, C.POINTER(WindowOpts), C.c_void_p, f64p, i32p, f64p, C.POINTER(C.c_int32),
                                   C.POINTER(H), C.POINTER(WindowInfo)]
    lib.lvba_window_split.argtypes = [C.c_int32, C.c_int32, C.c_int32, i32p]
    lib.lvba_window_ba_multi.argtypes = [C.c_int32, C.POINTER(H), f64p, C.POINTER(WindowOpts), C.c_void_p, f64p, i32p, f64p,
                                         C.POINTER(C.c_int32), C.POINTER(H), C.POINTER(WindowInfo)]
    lib.lvba_lidar_ba_default_opts.argtypes = [C.POINTER(LidarBaOpts)]
    lib.lvba_lidar_ba.argtypes = [H, f64p, C.POINTER(LidarBaOpts), f64p, C.POINTER(LidarBaReport)]
    lib.lvba_lidar_ba_multi.argtypes = [C.c_int32, C.POINTER(H), f64p, C.POINTER(LidarBaOpts), f64p, C.POINTER(LidarBaReport)]
    lib.lvba_lidar_ba_priors.argtypes = [H, f64p, C.POINTER(LidarBaOpts), C.c_int32, C.c_void_p, f64p, C.POINTER(LidarBaReport),
                                         C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lvba_lidar_ba_multi_priors.argtypes = [C.c_int32, C.POINTER(H), f64p, C.POINTER(LidarBaOpts), C.c_int32, C.c_void_p, f64p,
                                               C.POINTER(LidarBaReport), C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lvba_lidar_ba_robust.argtypes = [C.c_int32, C.POINTER(H), f64p, C.POINTER(LidarBaOpts), C.POINTER(Loss), C.POINTER(Loss), C.c_int32,
                                         C.c_void_p, f64p, C.POINTER(LidarBaReport), C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lvba_triangulate_tracks.argtypes = [C.c_int32, C.c_int32, C.c_int64, i64p, C.c_void_p, C.c_void_p, f64p, f64p, f64p, f64p,
                                            f64p, i32p, u8p]
    lib.lvba_depth_render.argtypes = [C.c_void_p, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p, C.c_int32, C.c_int32, C.c_double,
                                      C.c_double, C.POINTER(C.c_void_p)]
    lib.lvba_depth_upload.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, np.ctypeslib.ndpointer(np.float32, flags="C"),
                                      C.POINTER(C.c_void_p)]
    lib.lvba_depth_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lvba_depth_download.argtypes = [C.c_void_p, C.c_int32, np.ctypeslib.ndpointer(np.float32, flags="C")]
    lib.lvba_depth_destroy.argtypes = [C.c_void_p]
    lib.lvba_fuse_default_opts.argtypes = [C.POINTER(FuseOpts)]
    lib.lvba_fuse_tracks.argtypes = [C.c_int32, C.c_void_p, C.c_int32, f64p, f64p, f64p, C.c_int64, i64p, C.c_void_p, C.c_void_p,
                                     C.POINTER(FuseOpts), C.c_void_p, f64p, f64p, C.c_void_p]
    lib.lvba_colorize_default_opts.argtypes = [C.POINTER(ColorizeOpts)]
    lib.lvba_colorize_create.argtypes = [C.c_void_p, f64p, f64p, f64p, C.c_int32, C.c_int32, C.POINTER(ColorizeOpts),
                                         C.POINTER(C.c_void_p)]
    lib.lvba_colorize_add_images.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_colorize_count.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.lvba_colorize_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_colorize_profile.argtypes = [C.c_void_p, C.c_void_p]
    lib.lvba_colorize_destroy.argtypes = [C.c_void_p]
    lib.lvba_mapq_default_opts.argtypes = [C.POINTER(MapqOpts)]
    lib.lvba_mapq_scans.argtypes = [C.c_void_p, f64p, C.c_int32, C.c_int32, C.POINTER(MapqOpts), C.POINTER(MapqSummary), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_mapq_points.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.POINTER(MapqOpts), C.POINTER(MapqSummary), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_register_default_opts.argtypes = [C.POINTER(RegisterOpts)]
    lib.lvba_register_linearize.argtypes = [H, H, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(RegisterOpts), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    lib.lvba_register_scans.argtypes = [H, H, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(RegisterOpts), C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    lib.lvba_submaps_build.argtypes = [H, C.c_int32, C.c_int32, C.c_int32, f64p, C.POINTER(VoxelOpts), C.POINTER(H)]
    lib.lvba_submaps_count.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lvba_submaps_find_planes.argtypes = [H, C.c_int64, C.c_void_p, f64p, f64p, u8p]
    lib.lvba_register_linearize_submaps.argtypes = [H, H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RegisterOpts), C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_register_scans_submaps.argtypes = [H, H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RegisterOpts), C.c_void_p,
                                                C.c_void_p, C.c_void_p]
    lib.lvba_loop_default_opts.argtypes = [C.POINTER(LoopOpts)]
    lib.lvba_loop_candidates.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.POINTER(LoopOpts), C.c_int64, C.c_void_p,
                                         C.POINTER(C.c_int64)]
    lib.lvba_place_default_opts.argtypes = [C.POINTER(PlaceOpts)]
    lib.lvba_place_descriptors.argtypes = [H, C.c_int32, C.c_int32, C.POINTER(PlaceOpts), C.c_void_p, C.c_void_p]
    lib.lvba_place_search.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.POINTER(PlaceOpts), C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
    lib.lvba_place_candidates.argtypes = [H, C.POINTER(PlaceOpts), C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
    lib.lvba_closure_default_opts.argtypes = [C.POINTER(ClosureOpts)]
    lib.lvba_closure_consistency.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(ClosureOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.lvba_posegraph_default_opts.argtypes = [C.POINTER(PosegraphOpts)]
    lib.lvba_posegraph_relax.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(PosegraphOpts), C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PosegraphReport)]
    lib.lvba_match_default_opts.argtypes = [C.POINTER(MatchOpts)]
    lib.lvba_match_create.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(H)]
    lib.lvba_match_destroy.argtypes = [H]
    lib.lvba_match_set_geometry.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_match_pairs.argtypes = [H, C.c_int64, C.c_void_p, C.POINTER(MatchOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    lib.lvba_match_scan.argtypes = [H, C.c_int32, C.c_int32, C.POINTER(MatchOpts), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_match_set_depth.argtypes = [H, C.c_void_p]
    lib.lvba_match_points.argtypes = [H, C.c_void_p]
    lib.lvba_covis_default_opts.argtypes = [C.POINTER(CovisOpts)]
    lib.lvba_covis_samples.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CovisOpts), C.c_void_p]
    lib.lvba_covis_counts.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CovisOpts), C.c_void_p, C.c_void_p]
    lib.lvba_covis_pairs.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CovisOpts), C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    lib.lvba_trackgraph_create.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.POINTER(H), C.POINTER(TrackGraphInfo)]
    lib.lvba_trackgraph_components.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_trackgraph_orders.argtypes = [H, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_trackgraph_destroy.argtypes = [H]
    lib.lvba_verify_default_opts.argtypes = [C.POINTER(VerifyOpts)]
    lib.lvba_verify_create.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(H)]
    lib.lvba_verify_destroy.argtypes = [H]
    lib.lvba_verify_pairs.argtypes = [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(VerifyOpts), C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_verify_hypotheses.argtypes = [H, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(VerifyOpts), C.c_void_p, C.c_void_p]
    lib.lvba_verify_score.argtypes = [H, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.lvba_verify_pairs_model.argtypes = [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(VerifyOpts), C.c_int32, C.c_double,
                                            C.c_int64] + [C.c_void_p] * 9
    lib.lvba_verify_hypotheses_homography.argtypes = lib.lvba_verify_hypotheses.argtypes
    lib.lvba_verify_score_homography.argtypes = lib.lvba_verify_score.argtypes
    lib.lvba_sift_default_opts.argtypes = [C.POINTER(SiftOpts)]
    lib.lvba_sift_tile_width.argtypes = []
    lib.lvba_sift_blur_taps.argtypes = [C.POINTER(SiftOpts), C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
    lib.lvba_sift_extract.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(SiftOpts), C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_sift_profile.argtypes = [C.c_void_p]
    lib.lvba_sift_pyramid.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(SiftOpts), C.c_int32, C.c_void_p,
                                      C.c_void_p]
    lib.lvba_sift_candidates.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(SiftOpts), C.c_int64, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_int64)]
    lib.lvba_dynamic_default_opts.argtypes = [C.POINTER(DynamicOpts)]
    lib.lvba_dynamic_labels.argtypes = [C.c_void_p, f64p, C.c_int32, C.c_int32, C.POINTER(DynamicOpts), C.POINTER(DynamicSummary),
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_scans_select.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(H)]
    lib.lvba_scans_info.argtypes = [H, C.POINTER(C.c_int32), C.c_void_p]
    lib.lvba_scans_download.argtypes = [H, C.c_int32, np.ctypeslib.ndpointer(np.float32, flags="C")]
    lib.lvba_resect_default_opts.argtypes = [C.POINTER(ResectOpts)]
    lib.lvba_resect_images.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ResectOpts),
                                       C.c_int64] + [C.c_void_p] * 9
    lib.lvba_resect_hypotheses.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ResectOpts), C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    lib.lvba_resect_score.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.lvba_resect_lift.argtypes = [H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_calib_default_opts.argtypes = [C.POINTER(CalibOpts)]
    _calib = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
              C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(CalibOpts)]
    lib.lvba_calib_extrinsic.argtypes = _calib + [C.c_void_p] * 11
    lib.lvba_calib_linearize.argtypes = _calib + [C.c_void_p] * 5
    lib.lvba_calib_td_default_opts.argtypes = [C.POINTER(CalibTdOpts)]
    # lvba_calib_*'s arguments with body_twists after body_poses and td0 after tci
    _calib_td = _calib[:3] + [C.c_void_p] + _calib[3:14] + [C.c_void_p, C.POINTER(CalibTdOpts)]
    lib.lvba_calib_extrinsic_td.argtypes = _calib_td + [C.c_void_p] * 12
    lib.lvba_calib_linearize_td.argtypes = _calib_td + [C.c_void_p] * 5
    lib.lvba_photo_default_opts.argtypes = [C.POINTER(PhotoOpts)]
    lib.lvba_photo_create.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.POINTER(PhotoOpts), C.POINTER(H)]
    lib.lvba_photo_add_images.argtypes = [H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_photo_finish.argtypes = [H, C.POINTER(PhotoSummary), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_photo_sums.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_photo_free.argtypes = [H]
    lib.lvba_photo_free.restype = None
    lib.lvba_palign_default_opts.argtypes = [C.POINTER(PalignOpts)]
    lib.lvba_palign_create.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.POINTER(PalignOpts), C.POINTER(H)]
    _palign = [H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_palign_linearize.argtypes = _palign + [C.c_void_p]
    lib.lvba_palign_align.argtypes = _palign + [C.c_void_p] * 10
    lib.lvba_palign_profile.argtypes = [H, C.c_void_p]
    lib.lvba_palign_free.argtypes = [H]
    lib.lvba_palign_free.restype = None
    lib.lvba_expo_default_opts.argtypes = [C.POINTER(ExpoOpts)]
    lib.lvba_expo_create.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.POINTER(ExpoOpts), C.POINTER(H)]
    lib.lvba_expo_sums.argtypes = _palign + [C.c_void_p, C.c_void_p]
    lib.lvba_expo_solve.argtypes = [C.c_int32, C.c_void_p, C.POINTER(ExpoOpts), C.c_void_p, C.c_void_p]
    lib.lvba_expo_profile.argtypes = [H, C.c_void_p]
    lib.lvba_expo_free.argtypes = [H]
    lib.lvba_expo_free.restype = None
    lib.lvba_photo_add_images_gains.argtypes = _palign + [C.c_void_p]
    lib.lvba_undistort_default_opts.argtypes = [C.POINTER(UndistortOpts)]
    lib.lvba_undistort_tile.argtypes = [C.POINTER(C.c_int32)] * 3
    lib.lvba_undistort_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(UndistortOpts), C.POINTER(H)]
    lib.lvba_undistort_info.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64)]
    lib.lvba_undistort_images.argtypes = [H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lvba_undistort_map.argtypes = [H, C.c_void_p, C.c_void_p]
    lib.lvba_undistort_profile.argtypes = [H, C.c_void_p]
    lib.lvba_undistort_free.argtypes = [H]
    lib.lvba_undistort_free.restype = None
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if name.endswith("_default_opts") or name in ("lvba_depth_destroy", "lvba_colorize_destroy"):     # these return void
            fn.restype = None
        elif fn.restype is C.c_int:  # default
            fn.restype = C.c_int32
    _lib = lib
    return lib


def flatten_rows(arrays, dtype, width):
    """(flat [total, width] of `dtype`, off int64 [n + 1]): per-image or per-pair arrays, each [n_i, width], back to back"""
    rows = [np.asarray(a, dtype).reshape(-1, width) for a in arrays]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, width), dtype)
    return flat, off


def check(rc, allow_numeric=False):
    if rc == OK or (allow_numeric and rc > 0):
        return rc
    raise LvbaError(rc, load().lvba_last_error().decode(errors="replace"))
