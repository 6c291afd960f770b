"""The C ABI of libmpsfm_hip.so as Python sees it: declared here once, checked against the headers by tests/test_abi_cpu.py.

* every ``ctypes.Structure`` mirror of a struct of include/mpsfm_hip.h; ``_c_name_`` names the C struct;
* ``SIGNATURES``: restype and argtypes of every function of include/mpsfm_hip.h;
* ``DEBUG_SIGNATURES``: the same for the test and diagnostic hooks of include/mpsfm_hip_debug.h;
* ``lib()``: loads the library and applies both tables, once.

A new entry point is a prototype in the header, an entry in the table and, for a new struct, a class here; the test fails until the
three agree.  This module imports nothing of the package, so every other module may import it.
"""

from __future__ import annotations

import ctypes as C
import os

MAX_TRACE = 64  # MPSFM_MAX_TRACE
INT_MAX_IRLS = 16  # MPSFM_INT_MAX_IRLS

TERMINATION_NAMES = {
    0: "function_tolerance",
    1: "gradient_tolerance",
    2: "parameter_tolerance",
    3: "max_iterations",
    4: "min_radius",
    5: "invalid_steps",
    6: "no_variables",
}

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_void_p)  # mpsfm_allreduce_fn


# ---- structs -------------------------------------------------------------------------------------------------------------------
class CProblem(C.Structure):
    _c_name_ = "mpsfm_ba_problem"
    _fields_ = [
        ("n_cams", C.c_int32), ("n_pts", C.c_int32), ("n_intr", C.c_int32), ("cam_intr", C.c_void_p), ("cam_intr_idx", C.c_void_p),
        ("pose_const", C.c_void_p), ("gauge_axis_cam", C.c_int32), ("pt_const", C.c_void_p), ("n_obs", C.c_int64),
        ("obs_cam", C.c_void_p), ("obs_pt", C.c_void_p), ("obs_xy", C.c_void_p), ("reproj_loss_type", C.c_int32),
        ("reproj_loss_scale", C.c_double), ("reproj_loss_magnitude", C.c_double), ("n_dobs", C.c_int64), ("dobs_cam", C.c_void_p),
        ("dobs_pt", C.c_void_p), ("dobs_depth", C.c_void_p), ("dobs_magnitude", C.c_void_p), ("dobs_param", C.c_void_p),
        ("depth_loss_type", C.c_int32), ("shift_logscale", C.c_void_p),
    ]


class CState(C.Structure):
    _c_name_ = "mpsfm_ba_state"
    _fields_ = [("cam_quat_xyzw", C.c_void_p), ("cam_t", C.c_void_p), ("pts", C.c_void_p)]


class COptions(C.Structure):
    _c_name_ = "mpsfm_ba_options"
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double), ("max_num_consecutive_invalid_steps", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("device", C.c_int32), ("stream", C.c_void_p), ("verbose", C.c_int32), ("allreduce", ALLREDUCE_FN),
        ("allreduce_user", C.c_void_p), ("world_size", C.c_int32), ("rank", C.c_int32), ("use_rccl", C.c_int32),
        ("comm_id", C.c_uint8 * 128),
    ]


class CSummary(C.Structure):
    _c_name_ = "mpsfm_ba_summary"
    _fields_ = [
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("fixed_cost", C.c_double), ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32), ("termination", C.c_int32),
        ("num_residual_blocks", C.c_int64), ("num_residual_evals", C.c_int64), ("num_jacobian_evals", C.c_int64),
        ("reduced_dim", C.c_int32), ("final_radius", C.c_double), ("time_total_s", C.c_double), ("time_linearize_s", C.c_double),
        ("time_dense_s", C.c_double), ("time_update_s", C.c_double), ("trace_len", C.c_int32),
        ("trace_cost", C.c_double * MAX_TRACE), ("trace_radius", C.c_double * MAX_TRACE), ("trace_accepted", C.c_uint8 * MAX_TRACE),
    ]

    def to_dict(self) -> dict:
        n = self.trace_len
        return {
            "initial_cost": self.initial_cost,
            "final_cost": self.final_cost,
            "fixed_cost": self.fixed_cost,
            "num_iterations": self.num_iterations,
            "num_successful_steps": self.num_successful_steps,
            "num_unsuccessful_steps": self.num_unsuccessful_steps,
            "termination": TERMINATION_NAMES.get(self.termination, str(self.termination)),
            "num_residual_blocks": self.num_residual_blocks,
            "num_residual_evals": self.num_residual_evals,
            "num_jacobian_evals": self.num_jacobian_evals,
            "reduced_dim": self.reduced_dim,
            "final_radius": self.final_radius,
            "time_total_s": self.time_total_s,
            "time_linearize_s": self.time_linearize_s,
            "time_dense_s": self.time_dense_s,
            "time_update_s": self.time_update_s,
            "trace_cost": [self.trace_cost[i] for i in range(n)],
            "trace_radius": [self.trace_radius[i] for i in range(n)],
            "trace_accepted": [int(self.trace_accepted[i]) for i in range(n)],
        }


class CTracks(C.Structure):
    _c_name_ = "mpsfm_tracks"
    _fields_ = [
        ("n_cams", C.c_int32), ("n_tracks", C.c_int32), ("n_intr", C.c_int32), ("cam_quat_xyzw", C.c_void_p), ("cam_t", C.c_void_p),
        ("cam_intr", C.c_void_p), ("cam_intr_idx", C.c_void_p), ("track_start", C.c_void_p), ("el_cam", C.c_void_p),
        ("el_xy", C.c_void_p),
    ]


class CLiftMaps(C.Structure):
    _c_name_ = "mpsfm_lift_maps"
    _fields_ = [("activated", C.c_void_p), ("map_h", C.c_void_p), ("map_w", C.c_void_p), ("depth_map", C.c_void_p),
                ("valid_map", C.c_void_p), ("sx", C.c_void_p), ("sy", C.c_void_p)]


class CLiftInfo(C.Structure):
    _c_name_ = "mpsfm_lift_info"
    _fields_ = [("n_risky", C.c_int64), ("n_lifted", C.c_int64), ("n_no_lift", C.c_int64), ("n_maps_uploaded", C.c_int32),
                ("bytes_uploaded", C.c_int64), ("ms", C.c_double)]


class CIntProblem(C.Structure):
    _c_name_ = "mpsfm_int_problem"
    _fields_ = [
        ("H", C.c_int32), ("W", C.c_int32),
        ("depth_prior", C.c_void_p), ("depth_uncertainty", C.c_void_p), ("valid", C.c_void_p), ("normals", C.c_void_p),
        ("normals_var", C.c_void_p), ("depth_init", C.c_void_p), ("K", C.c_double * 4),
        ("n_sparse", C.c_int32), ("sparse_x", C.c_void_p), ("sparse_y", C.c_void_p), ("sparse_depth3d", C.c_void_p),
        ("sparse_zvar", C.c_void_p),
        ("large_number", C.c_double), ("tol", C.c_double), ("step_size", C.c_double), ("cg_tol", C.c_double),
        ("lambda1", C.c_double), ("lambda2", C.c_double), ("k", C.c_double), ("depth_magnitude_multiplier", C.c_double),
        ("normals_magnitude_multiplier", C.c_double), ("scale_filter_factor", C.c_double),
        ("max_iter", C.c_int32), ("cg_max_iter", C.c_int32), ("scale_filter", C.c_int32),
        ("init", C.c_int32), ("integrated", C.c_int32), ("energy_old", C.c_double), ("wu", C.c_void_p), ("wv", C.c_void_p),
    ]


class CIntSummary(C.Structure):
    _c_name_ = "mpsfm_int_summary"
    _fields_ = [
        ("changed", C.c_int32), ("irls_iterations", C.c_int32), ("cg_iterations_total", C.c_int32), ("integrated_out", C.c_int32),
        ("energy_initial", C.c_double), ("energy_final", C.c_double), ("energy_old_out", C.c_double),
        ("cg_iters", C.c_int32 * INT_MAX_IRLS), ("energies", C.c_double * (INT_MAX_IRLS + 1)), ("ms", C.c_float),
    ]


class CTriOptions(C.Structure):
    _c_name_ = "mpsfm_tri_options"
    _fields_ = [("max_transitivity", C.c_int32), ("create_max_angle_error", C.c_double), ("continue_max_angle_error", C.c_double),
                ("merge_max_reproj_error", C.c_double), ("complete_max_reproj_error", C.c_double), ("complete_max_transitivity", C.c_int32),
                ("re_max_angle_error", C.c_double), ("re_min_ratio", C.c_double), ("re_max_trials", C.c_int32), ("min_angle", C.c_double),
                ("ignore_two_view_tracks", C.c_int32)]


class CTriGraph(C.Structure):
    _c_name_ = "mpsfm_tri_graph"
    _fields_ = [("n_images", C.c_int32), ("kp_start", C.c_void_p), ("kp_xy", C.c_void_p), ("cam_intr", C.c_void_p),
                ("corr_start", C.c_void_p), ("corr_kp", C.c_void_p)]


class CTriState(C.Structure):
    _c_name_ = "mpsfm_tri_state"
    _fields_ = [("registered", C.c_void_p), ("cam_quat_xyzw", C.c_void_p), ("cam_t", C.c_void_p), ("kp_point", C.c_void_p),
                ("n_points", C.c_int64), ("xyz", C.c_void_p)]


class CDepthGather(C.Structure):
    _c_name_ = "mpsfm_depth_gather"
    _fields_ = [
        ("n_images", C.c_int32), ("map_h", C.c_void_p), ("map_w", C.c_void_p), ("depth_map", C.c_void_p), ("valid_map", C.c_void_p),
        ("sx", C.c_void_p), ("sy", C.c_void_p), ("cam_quat_xyzw", C.c_void_p), ("cam_t", C.c_void_p),
        ("n_obs", C.c_int64), ("obs_img", C.c_void_p), ("obs_xy", C.c_void_p), ("obs_var", C.c_void_p), ("obs_pt", C.c_void_p),
        ("n_pts", C.c_int32), ("pts", C.c_void_p),
        ("scale_filter", C.c_int32), ("scale_filter_factor", C.c_double), ("gross_outliers", C.c_int32), ("multiplier", C.c_double),
    ]


class CTriCandidates(C.Structure):
    _c_name_ = "mpsfm_tri_candidates"
    _fields_ = [("n_candidates", C.c_int64), ("cand_start", C.c_void_p), ("view_cam_from_world", C.c_void_p), ("view_intr", C.c_void_p),
                ("view_xy", C.c_void_p), ("min_tri_angle", C.c_double), ("max_error", C.c_double), ("residual_type", C.c_int32),
                ("min_num_trials", C.c_void_p)]


class CDcImage(C.Structure):
    _c_name_ = "mpsfm_dc_image"
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("depth", C.c_void_p), ("variance", C.c_void_p),
                ("prior_std_multiplier", C.c_double), ("intr_scaled", C.c_double * 4), ("intr", C.c_double * 4),
                ("cam_from_world", C.c_double * 12)]


class CDcSummary(C.Structure):
    _c_name_ = "mpsfm_dc_summary"
    _fields_ = [("ms", C.c_float), ("n_legs", C.c_int32), ("n_pixels", C.c_int64)]


class CRansacOptions(C.Structure):
    _c_name_ = "mpsfm_ransac_options"
    """mpsfm_ransac_options: the options of both LO-RANSAC estimators."""
    _fields_ = [("max_error", C.c_double), ("min_inlier_ratio", C.c_double), ("confidence", C.c_double),
                ("dyn_num_trials_multiplier", C.c_double), ("min_num_trials", C.c_int64), ("max_num_trials", C.c_int64),
                ("seed", C.c_uint64), ("batch_trials", C.c_int32), ("reserved", C.c_int32)]


CAbsPoseOptions = CRelPoseOptions = CAlign3dOptions = CRansacOptions  # typedefs of mpsfm_ransac_options in the header


class CAbsPoseResult(C.Structure):
    _c_name_ = "mpsfm_abs_pose_result"
    _fields_ = [("cam_from_world", C.c_double * 12), ("num_inliers", C.c_int64), ("num_trials", C.c_int64), ("max_num_trials", C.c_int64),
                ("num_models", C.c_int64), ("success", C.c_int32), ("lo_rounds", C.c_int32), ("num_batches", C.c_int32), ("ms", C.c_float)]


class CAlign3dResult(C.Structure):
    _c_name_ = "mpsfm_align3d_result"
    _fields_ = [("tgt_from_src", C.c_double * 12), ("scale", C.c_double), ("num_inliers", C.c_int64), ("num_trials", C.c_int64),
                ("max_num_trials", C.c_int64), ("num_models", C.c_int64), ("success", C.c_int32), ("lo_rounds", C.c_int32),
                ("num_batches", C.c_int32), ("ms", C.c_float)]


class CIcpOptions(C.Structure):
    _c_name_ = "mpsfm_icp_options"
    _fields_ = [("max_distance", C.c_double), ("max_angle_deg", C.c_double), ("edge_ratio", C.c_double), ("eps_rotation", C.c_double),
                ("eps_translation", C.c_double), ("max_iterations", C.c_int32), ("min_pairs", C.c_int32), ("stride", C.c_int32),
                ("reserved", C.c_int32)]


class CIcpResult(C.Structure):
    _c_name_ = "mpsfm_icp_result"
    _fields_ = [("tgt_from_src", C.c_double * 12), ("scale", C.c_double), ("info", C.c_double * 36), ("rhs", C.c_double * 6),
                ("rmse", C.c_double), ("num_pairs", C.c_int64), ("rejected", C.c_int64 * 4), ("iterations", C.c_int32),
                ("status", C.c_int32), ("ms", C.c_float), ("reserved", C.c_int32)]


class CRelPoseResult(C.Structure):
    _c_name_ = "mpsfm_rel_pose_result"
    _fields_ = [("E", C.c_double * 9), ("cam2_from_cam1", C.c_double * 12), ("num_inliers", C.c_int64), ("num_trials", C.c_int64),
                ("max_num_trials", C.c_int64), ("num_models", C.c_int64), ("lo_rounds", C.c_int64), ("num_batches", C.c_int64),
                ("num_cheirality_points", C.c_int64), ("success", C.c_int32), ("ms", C.c_float)]


class CTwoViewOptions(C.Structure):
    _c_name_ = "mpsfm_two_view_options"
    _fields_ = [("ransac", CRansacOptions), ("min_num_inliers", C.c_int64), ("min_E_F_inlier_ratio", C.c_double),
                ("max_H_inlier_ratio", C.c_double), ("watermark_min_inlier_ratio", C.c_double), ("watermark_border_size", C.c_double),
                ("detect_watermark", C.c_int32), ("compute_relative_pose", C.c_int32)]


class CTwoViewLeg(C.Structure):
    _c_name_ = "mpsfm_two_view_leg"
    _fields_ = [("num_inliers", C.c_int64), ("num_trials", C.c_int64), ("max_num_trials", C.c_int64), ("lo_rounds", C.c_int64),
                ("num_batches", C.c_int64), ("success", C.c_int32), ("reserved", C.c_int32)]


class CTwoViewResult(C.Structure):
    _c_name_ = "mpsfm_two_view_result"
    _fields_ = [("E", C.c_double * 9), ("F", C.c_double * 9), ("H", C.c_double * 9), ("cam2_from_cam1", C.c_double * 12),
                ("tri_angle", C.c_double), ("leg", CTwoViewLeg * 4), ("num_inliers", C.c_int64), ("num_cheirality_points", C.c_int64),
                ("num_border_inliers", C.c_int64), ("config", C.c_int32), ("success", C.c_int32), ("watermark", C.c_int32),
                ("ms", C.c_float)]


class CTwoViewBatchReport(C.Structure):
    _c_name_ = "mpsfm_two_view_batch_report"
    _fields_ = [("num_groups", C.c_int64), ("num_syncs", C.c_int64), ("num_launches", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]


class CRegImage(C.Structure):
    _c_name_ = "mpsfm_reg_image"
    _fields_ = [("map_h", C.c_int32), ("map_w", C.c_int32), ("depth_map", C.c_void_p), ("sx", C.c_double), ("sy", C.c_double),
                ("intr", C.c_double * 4), ("quat_xyzw", C.c_double * 4), ("t", C.c_double * 3)]


class CInitPair(C.Structure):
    _c_name_ = "mpsfm_init_pair"
    _fields_ = [("n_matches", C.c_int64), ("xy1", C.c_void_p), ("xy2", C.c_void_p), ("select", C.c_void_p),
                ("intr1", C.c_double * 4), ("intr2", C.c_double * 4), ("cam2_from_cam1", C.c_double * 12),
                ("map_h", C.c_int32), ("map_w", C.c_int32), ("prior_map", C.c_void_p), ("valid_map", C.c_void_p),
                ("sx", C.c_double), ("sy", C.c_double), ("rescale", C.c_double), ("tri_min_angle", C.c_double),
                ("tri_max_error", C.c_double), ("what", C.c_int32), ("reserved", C.c_int32)]


class CInitCandidates(C.Structure):
    _c_name_ = "mpsfm_init_candidates"
    _fields_ = [("flags", C.c_void_p), ("tri_xyz", C.c_void_p), ("tri_angle_deg", C.c_void_p), ("lift_xyz", C.c_void_p),
                ("lift_angle_deg", C.c_void_p), ("d_prior", C.c_void_p), ("ms", C.c_float)]


class CNmsInfo(C.Structure):
    _c_name_ = "mpsfm_nms_info"
    _fields_ = [("rounds", C.c_int32), ("launches", C.c_int32), ("cells", C.c_int32), ("max_cell_points", C.c_int32), ("ms", C.c_float),
                ("reserved", C.c_int32)]


class CMatchOptions(C.Structure):
    _c_name_ = "mpsfm_match_options"
    _fields_ = [("ratio_threshold", C.c_double), ("distance_threshold", C.c_double), ("score_threshold", C.c_double),
                ("mutual_check", C.c_int32), ("inputs_on_device", C.c_int32), ("stream", C.c_void_p)]


class CMatchInfo(C.Structure):
    _c_name_ = "mpsfm_match_info"
    _fields_ = [("num_matches", C.c_int64), ("ms", C.c_float), ("column_ranges", C.c_int32)]


class CMatchBatchReport(C.Structure):
    _c_name_ = "mpsfm_match_batch_report"
    _fields_ = [("num_matches", C.c_int64), ("num_groups", C.c_int64), ("num_launches", C.c_int64), ("num_syncs", C.c_int64),
                ("num_workgroups", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]


class CRetrievalOptions(C.Structure):
    _c_name_ = "mpsfm_retrieval_options"
    _fields_ = [("num_select", C.c_int32), ("use_min_score", C.c_int32), ("min_score", C.c_double), ("column_ranges", C.c_int32),
                ("inputs_on_device", C.c_int32), ("stream", C.c_void_p)]


class CRetrievalInfo(C.Structure):
    _c_name_ = "mpsfm_retrieval_info"
    _fields_ = [("num_pairs", C.c_int64), ("num_launches", C.c_int64), ("num_syncs", C.c_int64), ("ms", C.c_float),
                ("column_ranges", C.c_int32)]


class CCorrGraphInfo(C.Structure):
    _c_name_ = "mpsfm_corr_graph_info"
    _fields_ = [("num_added", C.c_int64), ("num_invalid", C.c_int64), ("num_self_pairs", C.c_int64), ("num_duplicates", C.c_int64),
                ("num_launches", C.c_int64), ("num_syncs", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]


class CSceneQueryInfo(C.Structure):
    _c_name_ = "mpsfm_scene_query_info"
    _fields_ = [("num_launches", C.c_int64), ("num_syncs", C.c_int64), ("num_groups", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]


class CSceneFilterOptions(C.Structure):
    _c_name_ = "mpsfm_scene_filter_options"
    _fields_ = [("max_reproj_error", C.c_double), ("min_tri_angle_rad", C.c_double), ("risky_min_tri_angle_rad", C.c_double),
                ("negative_depth", C.c_int32), ("reserved", C.c_int32)]


class CSceneFilterInfo(C.Structure):
    _c_name_ = "mpsfm_scene_filter_info"
    _fields_ = [("num_negative", C.c_int64), ("num_changed_a", C.c_int64), ("num_changed_b", C.c_int64), ("n_points_deleted", C.c_int64),
                ("n_observations_deleted", C.c_int64), ("num_syncs", C.c_int64), ("ms", C.c_float),
                ("ms_tracks", C.c_float)]


class CRecipOptions(C.Structure):
    _c_name_ = "mpsfm_recip_options"
    _fields_ = [("subsample", C.c_int32), ("max_iter", C.c_int32), ("inputs_on_device", C.c_int32), ("stream", C.c_void_p)]


class CRecipInfo(C.Structure):
    _c_name_ = "mpsfm_recip_info"
    _fields_ = [("n_seeds", C.c_int64), ("n_converged", C.c_int64), ("nn_queries", C.c_int64), ("iterations", C.c_int32),
                ("column_ranges", C.c_int32), ("ms", C.c_float), ("reserved", C.c_int32)]


class CWarpOptions(C.Structure):
    _c_name_ = "mpsfm_warp_options"
    _fields_ = [("sample_thresh", C.c_double), ("max_error", C.c_double), ("scale0", C.c_double * 2), ("scale1", C.c_double * 2),
                ("nms_radius", C.c_int32), ("inputs_on_device", C.c_int32), ("stream", C.c_void_p)]


class CWarpInfo(C.Structure):
    _c_name_ = "mpsfm_warp_info"
    _fields_ = [("num_dense", C.c_int64), ("num_valid", C.c_int64), ("num_matches", C.c_int64), ("ms", C.c_float), ("reserved", C.c_int32)]


class CDepthPriorConf(C.Structure):
    _c_name_ = "mpsfm_depth_prior_conf"
    _fields_ = [("inherent_noise", C.c_double), ("std_multiplier", C.c_double), ("prior_std_multiplier", C.c_double),
                ("max_std", C.c_double), ("depth_lim", C.c_double), ("fixed_uncertainty_val", C.c_double),
                ("depth_uncertainty", C.c_double), ("has_max_std", C.c_int32), ("has_depth_lim", C.c_int32),
                ("has_depth_uncertainty", C.c_int32), ("use_continuity", C.c_int32), ("fixed_uncertainty", C.c_int32),
                ("prior_uncertainty", C.c_int32), ("flip_consistency", C.c_int32), ("reserved", C.c_int32)]


class CDepthPriorProblem(C.Structure):
    _c_name_ = "mpsfm_depth_prior_problem"
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("int_height", C.c_int32), ("int_width", C.c_int32),
                ("mask_height", C.c_int32), ("mask_width", C.c_int32), ("is_float32", C.c_int32), ("n_kps", C.c_int32),
                ("depth", C.c_void_p), ("depth2", C.c_void_p), ("depth_variance", C.c_void_p), ("depth_variance2", C.c_void_p),
                ("valid", C.c_void_p), ("valid2", C.c_void_p), ("mask", C.c_void_p), ("kps", C.c_void_p),
                ("sx", C.c_double), ("sy", C.c_double)]


class CDepthPriorOutput(C.Structure):
    _c_name_ = "mpsfm_depth_prior_output"
    _fields_ = [("data_prior", C.c_void_p), ("uncertainty", C.c_void_p), ("valid", C.c_void_p), ("continuity_mask", C.c_void_p),
                ("uncertainty_update", C.c_void_p)]


class CNormalPriorConf(C.Structure):
    _c_name_ = "mpsfm_normal_prior_conf"
    _fields_ = [("inherent_polar_noise", C.c_double), ("std_multiplier", C.c_double), ("lc_std_multiplier", C.c_double),
                ("prior_std_multiplier", C.c_double), ("downscale_factor", C.c_double), ("flip_consistency", C.c_int32),
                ("reserved", C.c_int32)]


class CNormalPriorProblem(C.Structure):
    _c_name_ = "mpsfm_normal_prior_problem"
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("int_height", C.c_int32), ("int_width", C.c_int32),
                ("mask_height", C.c_int32), ("mask_width", C.c_int32), ("half_height", C.c_int32), ("half_width", C.c_int32),
                ("is_float32", C.c_int32), ("reserved", C.c_int32), ("normals", C.c_void_p), ("normals2", C.c_void_p), ("normals_variance", C.c_void_p),
                ("normals2_variance", C.c_void_p), ("mask", C.c_void_p), ("continuity_mask", C.c_void_p)]


class CNormalPriorOutput(C.Structure):
    _c_name_ = "mpsfm_normal_prior_output"
    _fields_ = [("data", C.c_void_p), ("uncertainty", C.c_void_p), ("data_downscaled", C.c_void_p),
                ("uncertainty_downscaled", C.c_void_p)]


class CPriorSummary(C.Structure):
    _c_name_ = "mpsfm_prior_summary"
    _fields_ = [("ms", C.c_float), ("n_images", C.c_int32), ("n_pixels", C.c_int64)]


# include/mpsfm_hip_debug.h: the Levenberg-Marquardt control block and its options as the decision kernels see them
LM_HEAD_DOUBLES = ("radius", "decrease_factor", "x_norm", "cur_cost", "fixed_cost", "initial_cost", "last_x_cost", "last_cand", "last_rel",
                   "last_step_norm", "last_mcc")
LM_HEAD_INTS = ("term", "iter", "invalid_run", "check_gradient", "accepted", "n_success", "n_unsuccess", "n_cost_evals", "n_jac_evals",
                "last_chol_fail", "trace_len", "pad_")


class CDebugLmCtl(C.Structure):
    _c_name_ = "mpsfm_debug_lm_ctl"
    _fields_ = ([(f, C.c_double) for f in LM_HEAD_DOUBLES] + [(f, C.c_int32) for f in LM_HEAD_INTS]
                + [("trace_cost", C.c_double * MAX_TRACE), ("trace_radius", C.c_double * MAX_TRACE), ("trace_accepted", C.c_uint8 * MAX_TRACE)])


class CDebugLmOpts(C.Structure):
    _c_name_ = "mpsfm_debug_lm_opts"
    _fields_ = [("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("min_relative_decrease", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double), ("max_iterations", C.c_int32),
                ("max_invalid_steps", C.c_int32)]


# ---- functions -----------------------------------------------------------------------------------------------------------------
# name -> (restype, argtypes).  Pointers are c_void_p (it takes byref(), addressof(), an array's .ctypes.data and None alike); the few
# POINTER(...) entries are out-parameters that every caller passes with byref().  `int` returns are the MPSFM_* status codes.
P, I32, I64, F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_f32p, _f64p, _i64p, _pp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_void_p)

SIGNATURES = {
    "mpsfm_abi_version": (C.c_int, []),
    "mpsfm_last_error": (C.c_char_p, []),
    "mpsfm_device_count": (C.c_int, []),
    "mpsfm_ba_default_options": (None, [P]),
    "mpsfm_comm_unique_id": (C.c_int, [P]),
    "mpsfm_ba_solve": (C.c_int, [P, P, P, P]),
    "mpsfm_ba_create": (C.c_int, [P, P, P, _pp]),
    "mpsfm_ba_set_state": (C.c_int, [P, P]),
    "mpsfm_ba_reset_state": (C.c_int, [P]),
    "mpsfm_ba_solve_resident": (C.c_int, [P, P]),
    "mpsfm_ba_get_state": (C.c_int, [P, P]),
    "mpsfm_ba_destroy": (None, [P]),
    "mpsfm_ba_eval_cost": (C.c_int, [P, _f64p, _f64p]),
    "mpsfm_ba_sweep_once": (C.c_int, [P, F64, _f32p]),
    "mpsfm_ba_sweep_parts": (C.c_int, [P, P, P]),
    "mpsfm_ba_get_reduced_system": (C.c_int, [P, P, P, I32]),
    "mpsfm_ba_reduced_dim": (C.c_int, [P]),
    "mpsfm_ba_get_dense_solution": (C.c_int, [P, P, I32]),
    "mpsfm_ba_dense_solve_once": (C.c_int, [P, _f32p]),
    "mpsfm_ba_dense_plan": (C.c_int, [P, P]),
    "mpsfm_point_covs": (C.c_int, [P, P, I32, P]),
    "mpsfm_triangulate_tracks": (C.c_int, [P, I32, P]),
    "mpsfm_filter_tracks": (C.c_int, [P, P, I32, P, P, P]),
    "mpsfm_lift_tracks": (C.c_int, [P, P, P, F64, I32, P, P, P, P, P, P]),
    "mpsfm_tri_default_options": (None, [P]),
    "mpsfm_triangulator_create": (C.c_int, [P, I32, _pp]),
    "mpsfm_triangulator_destroy": (None, [P]),
    "mpsfm_triangulator_set_state": (C.c_int, [P, P]),
    "mpsfm_triangulator_triangulate_image": (C.c_int, [P, P, I32, _i64p]),
    "mpsfm_triangulator_complete_image": (C.c_int, [P, P, I32, _i64p]),
    "mpsfm_triangulator_complete_tracks": (C.c_int, [P, P, P, I64, _i64p]),
    "mpsfm_triangulator_merge_tracks": (C.c_int, [P, P, P, I64, _i64p]),
    "mpsfm_triangulator_retriangulate": (C.c_int, [P, P, P, I32, _i64p]),
    "mpsfm_triangulator_num_ops": (I64, [P]),
    "mpsfm_triangulator_num_points": (I64, [P]),
    "mpsfm_triangulator_get_ops": (C.c_int, [P, P, P, P, P]),
    "mpsfm_triangulator_num_op_elements": (I64, [P]),
    "mpsfm_triangulator_get_op_elements": (C.c_int, [P, P]),
    "mpsfm_triangulator_stats": (C.c_int, [P, _i64p, _i64p, _i64p]),
    "mpsfm_tri_estimate_batch": (C.c_int, [P, I32, P, P, P]),
    "mpsfm_depth_blocks": (C.c_int, [P, I32, P, P, P, P, P, P]),
    "mpsfm_depth_stats": (C.c_int, [P, I32, P, P, P, P, I32, P, P, P, P, P, P, P, P]),
    "mpsfm_integrate_depth": (C.c_int, [P, I32, P, P]),
    "mpsfm_integrate_depth_batch": (C.c_int, [I32, P, I32, P, P]),
    "mpsfm_integration_variances": (C.c_int, [P, I32, I32, I32, P, P, F64, I32, P, P, P]),
    "mpsfm_depth_consistency": (C.c_int, [I32, P, I32, P, P, F64, F64, I32, P, P, P]),
    "mpsfm_abs_pose_estimate": (C.c_int, [I64, P, P, P, P, I32, P, P]),
    "mpsfm_rel_pose_estimate": (C.c_int, [I64, P, P, P, P, P, I32, P, P]),
    "mpsfm_two_view_default_options": (None, [P]),
    "mpsfm_two_view_geometry": (C.c_int, [I64, P, P, P, P, P, P, P, I32, P, P]),
    "mpsfm_two_view_geometry_batch": (C.c_int, [I64, P, P, P, P, P, P, P, P, I32, I32, P, P, P]),
    "mpsfm_registration_pairs": (C.c_int, [I32, P, I64, P, P, P, P, I32, P, I32, I32, P, P, P]),
    "mpsfm_init_pair_candidates": (C.c_int, [P, I32, P]),
    "mpsfm_radius_nms": (C.c_int, [I64, P, P, P, F64, I32, P, P, P]),
    "mpsfm_thin_dense_matches": (C.c_int, [I64, P, P, I64, P, P, P, F64, I32, I32, P, P, P]),
    "mpsfm_assign_keypoints": (C.c_int, [I64, P, I64, P, F64, I32, P, P]),
    "mpsfm_match_default_options": (None, [P]),
    "mpsfm_match_descriptors": (C.c_int, [I64, I64, I32, P, P, P, I32, P, P, P]),
    "mpsfm_match_descriptors_batch": (C.c_int, [I32, P, I32, P, I64, P, P, P, P, I32, I32, I32, P, P, P, P]),
    "mpsfm_match_map_descriptors": (C.c_int, [P, P, I32, I32, P, P, I32, I32, I32, I64, P, I64, P, P, I32, P, P, P]),
    "mpsfm_retrieval_default_options": (None, [P]),
    "mpsfm_retrieve_topk": (C.c_int, [I64, I64, I32, P, P, P, P, P, I32, P, P, P, P]),
    "mpsfm_recip_default_options": (None, [P]),
    "mpsfm_recip_seed_count": (I64, [I32, I32, I32]),
    "mpsfm_reciprocal_nns": (C.c_int, [P, I32, I32, P, I32, I32, I32, P, I32, I64, P, P, P, P]),
    "mpsfm_dense_correspondences": (C.c_int, [P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, P, I32, I64, P, P, P, P, P]),
    "mpsfm_warp_default_options": (None, [P]),
    "mpsfm_simple_nms": (C.c_int, [I32, I32, P, I32, I32, P, I32, P, P]),
    "mpsfm_kpids_to_matches0": (C.c_int, [I64, P, P, P, I64, I64, I32, P, I32, P, P, P, P]),
    "mpsfm_warp_matches": (C.c_int, [I32, I32, P, P, I32, I32, I32, I32, I32, P, I64, P, I64, P, I32, P, P, P, P, P, P, P, P]),
    "mpsfm_depth_priors": (C.c_int, [I32, P, P, I32, P, P]),
    "mpsfm_normal_priors": (C.c_int, [I32, P, P, I32, P, P]),
    "mpsfm_corr_graph_build": (C.c_int, [I32, P, I32, P, P, P, P, I32, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mpsfm_visibility_scores": (C.c_int, [I32, P, P, P, P, P, P, I32, I32, P, P, P, P]),
    "mpsfm_local_bundles": (C.c_int, [I32, P, P, I32, P, I32, F64, I32, P, P, P, P, P]),
    "mpsfm_filter_scene": (C.c_int, [P, P, P, P, P, P, I32, P, P, P, P, P, P]),
    "mpsfm_align3d_estimate": (C.c_int, [I64, P, P, I32, P, I32, P, P]),
    "mpsfm_align3d_fit": (C.c_int, [I64, P, P, P, I32, I32, P]),
    "mpsfm_lift_keypoints": (C.c_int, [I32, I32, P, P, I64, P, I32, P, P]),
    "mpsfm_depth_pair_register": (C.c_int, [I32, I32, P, P, I32, I32, P, P, I64, P, I64, P, I64, P, I32, P, I32, P, P, P, P, P]),
    "mpsfm_depth_normals": (C.c_int, [I32, I32, P, P, F64, I32, P, P]),
    "mpsfm_depth_pair_icp": (C.c_int, [I32, I32, P, P, I32, I32, P, P, P, F64, P, I32, P, P]),
    "mpsfm_depth_pair_register_dense": (C.c_int, [I32, I32, P, P, I32, I32, P, P, I64, P, I64, P, I64, P, I32, P, P, I32, P, P, P, P, P, P, P]),
}

# include/mpsfm_hip_debug.h: test and diagnostic hooks, outside the stable ABI
DEBUG_SIGNATURES = {
    "mpsfm_debug_set": (None, [C.c_int]),
    "mpsfm_debug_set_chol_trace": (C.c_int, [P]),
    "mpsfm_debug_panel_factor": (C.c_int, [P, C.c_int, P, C.POINTER(C.c_int)]),
    "mpsfm_debug_plan_create": (P, [P, I32, I32, I32, I32]),
    "mpsfm_debug_plan_destroy": (None, [P]),
    "mpsfm_debug_plan_get": (I64, [P, I32, P, I64]),
    "mpsfm_debug_host_cache": (I64, [I64, I32]),
    "mpsfm_debug_run_parts": (I64, [I32, I32]),
    "mpsfm_debug_graph_union": (C.c_int, [P, I32, I32, P]),
    "mpsfm_debug_pt_handoff": (C.c_int, [P]),
    "mpsfm_debug_direct_front": (C.c_int, [P]),
    "mpsfm_debug_direct_assemble": (C.c_int, [P, C.c_double, P, P, P, P, P]),
    "mpsfm_debug_dense_solve_given": (C.c_int, [P, P, P, I32, C.POINTER(I32)]),
    "mpsfm_debug_update_once": (C.c_int, [P, F64, P, I32, I32, P, P, P, P, I64, P, P, P]),
    "mpsfm_debug_read_trace": (C.c_int, [P, P, I64]),
    "mpsfm_debug_table": (I64, [P, I32, P, I64]),
    "mpsfm_debug_host_build": (I64, [P, I32, P, I64]),
    "mpsfm_debug_local_clocks": (C.c_int, [P, P]),
    "mpsfm_debug_local_skew": (C.c_int, [I32, I32, I64]),
    "mpsfm_debug_lm_decide": (C.c_int, [I32, P, P, P, P, P, P, I64, I32, P, P, P]),
    "mpsfm_debug_resources": (C.c_int, [I32, P]),
    "mpsfm_debug_math_probe": (C.c_int, [I32, P, I64, P]),
}


# ---- the library ---------------------------------------------------------------------------------------------------------------
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmpsfm_hip.so")

_lib = None


class MpsfmHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmpsfm_hip error {code}: {msg}")
        self.code = code


def lib():
    """Loads libmpsfm_hip.so (building it is __graft_entry__.build()'s job, not ours) and types every function of both tables."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MpsfmHipError(-2, f"{LIB_PATH} is missing: run `python -m mpsfm_amd.build` (hipcc, gfx950)")
        try:
            # torch wheels bundle their own libamdhip64; if ours (linked against /opt/rocm) is loaded
            # first the process ends up with two HIP runtimes and torch.cuda reports no devices.
            # Importing torch first makes its runtime the process-wide one (same soname).
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for table in (SIGNATURES, DEBUG_SIGNATURES):
            for name, (restype, argtypes) in table.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib
