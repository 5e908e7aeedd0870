"""ctypes binding of libsqrtlm.so (include/sqrtlm.h).

The library is the product: there is no CPU fallback. Importing works without
a GPU (the CPU test suite checks the exports), but creating a context on a
machine without a HIP device fails loudly with SQLM_ERR_NO_DEVICE.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SQLM_LIB_PATH selects a diagnostic build of the same library (libsqrtlm_prof.so)
LIB_PATH = os.environ.get("SQLM_LIB_PATH", os.path.join(_HERE, "libsqrtlm.so"))
TRACE_MAX = 256
NKERNEL_TIMERS = 9

SQLM_OK = 0
STATUS = {0: "ok", -1: "invalid argument", -2: "HIP runtime error", -3: "not SPD", -4: "out of device memory",
          -5: "aborted", -6: "no HIP device", -7: "state error", -8: "unsupported problem shape", -9: "RCCL error"}

# every symbol include/sqrtlm.h declares
EXPORTS = [
    "sqlm_version", "sqlm_status_string", "sqlm_ctx_create", "sqlm_ctx_destroy", "sqlm_set_problem",
    "sqlm_set_lidar", "sqlm_set_edge_level", "sqlm_set_robust", "sqlm_set_lidar_level", "sqlm_optimize",
    "sqlm_local_ba", "sqlm_global_ba", "sqlm_get_poses", "sqlm_get_points", "sqlm_get_edge_chi2",
    "sqlm_get_edge_depth_positive", "sqlm_get_edge_level", "sqlm_pose_from_Tcw_f32", "sqlm_pose_to_Tcw_f32",
    "sqlm_comm_id_size", "sqlm_comm_get_unique_id", "sqlm_ctx_set_comm", "sqlm_ctx_set_host_comm",
    "sqlm_ctx_set_host_p2p", "sqlm_ctx_set_comm_selfloop", "sqlm_comm_selftest", "sqlm_ctx_comm_info",
    "sqlm_bench_iterations",
    "sqlm_kernel_timer_name", "sqlm_debug_cr_levels", "sqlm_set_stereo",
    "sqlm_eg_set_problem", "sqlm_eg_optimize", "sqlm_eg_get_poses", "sqlm_eg_get_edge_chi2",
    "sqlm_eg_get_jacobians", "sqlm_eg_get_last_step", "sqlm_eg_get_exec_info",
    "sqlm_get_rcs_layout", "sqlm_get_exec_info", "sqlm_get_last_step",
    "sqlm_sim3_optimize", "sqlm_sim3_get_pair_chi2", "sqlm_sim3_get_linearization", "sqlm_sim3_get_last_step",
    "sqlm_pose_optimize", "sqlm_pose_refine_lidar", "sqlm_pose_get_edge_chi2", "sqlm_pose_get_linearization",
    "sqlm_pose_get_last_step",
    # int sqlm_lidar_associate(ctx, int n_map_clouds, const int64_t *map_off, const float *map_xyz,
    #     const float *map_Twc, int64_t n_query, const float *query_xyz, const float *query_Twc,
    #     double dist_sq_threshold, int32_t *nn_index, float *nn_sq_dist, float *nn_xyz, uint8_t *accepted,
    #     int64_t *n_pairs)
    # int sqlm_set_lidar_from_clouds(ctx, int32_t pose_index, <map and query arguments as above>,
    #     const float *query_normal, double info, double dist_sq_threshold, int64_t *n_pairs)
    # int sqlm_lidar_get_exec_info(ctx, int out[8])
    "sqlm_lidar_associate", "sqlm_set_lidar_from_clouds", "sqlm_lidar_get_exec_info",
    # int sqlm_get_lidar_error(ctx, double *err /* [n_lid] */)
    "sqlm_get_lidar_error",
    # int sqlm_set_lidar_kind(ctx, const uint8_t *kind /* [n_lid] 0 flat, 1 corner; NULL = flat */)
    # int sqlm_set_lidar_from_cloud_sets(ctx, int32_t pose_index, int n_sets, const sqlm_lidar_set *sets,
    #     int64_t *n_pairs /* [n_sets] */)
    "sqlm_set_lidar_kind", "sqlm_set_lidar_from_cloud_sets",
    # Sim3 RANSAC (Sim3Solver): every hypothesis of every candidate in one launch, and its host-only helpers
    "sqlm_sim3_ransac", "sqlm_sim3_ransac_get_inliers", "sqlm_sim3_ransac_get_hypothesis",
    "sqlm_sim3_ransac_max_its", "sqlm_sim3_ransac_scan", "sqlm_sim3_ransac_hypothesis_host",
    # PnP RANSAC (PnPsolver): every hypothesis of every candidate in one launch, the refines in a second
    "sqlm_pnp_ransac", "sqlm_pnp_ransac_get_inliers", "sqlm_pnp_ransac_get_refined", "sqlm_pnp_ransac_get_hypothesis",
    "sqlm_pnp_ransac_max_its", "sqlm_pnp_ransac_scan", "sqlm_pnp_ransac_hypothesis_host",
    "sqlm_pnp_ransac_refine_host",
    # LiDAR flat-feature extraction (Frame::lidarProcess, flat-point path) and its host twin
    "sqlm_lidar_features", "sqlm_lidar_features_host", "sqlm_lidar_features_get_state", "sqlm_lidar_features_info",
    "sqlm_lidar_feat_trig_probe",
    # both branches of Frame::ExtractFeaturePoints on one range image (the corner branch, Frame.cc:861-1038)
    "sqlm_lidar_features_all", "sqlm_lidar_features_all_host", "sqlm_lidar_features_all_get_state",
    "sqlm_lidar_features_all_info", "sqlm_lidar_corner_trig_probe", "sqlm_lidar_corner_angle_probe",
    # LiDAR depth image and keypoint depth association (Frame.cc:290-313, :333-408) and its host twin
    "sqlm_lidar_depth", "sqlm_lidar_depth_host", "sqlm_lidar_depth_get_state", "sqlm_lidar_depth_info",
]
# every symbol include/sqrtlm_capture.h declares
CAPTURE_EXPORTS = ["sqlm_capture_write", "sqlm_capture_read", "sqlm_capture_free", "sqlm_capture_replay",
                   "sqlm_save_trajectory_kitti"]
# every symbol include/sqrtlm_orb.h declares
ORB_EXPORTS = ["sqlm_orb_extract", "sqlm_orb_get_level", "sqlm_orb_match_bf", "sqlm_orb_search_for_init",
               "sqlm_orb_search_by_projection_local", "sqlm_orb_search_by_projection_last",
               "sqlm_orb_search_by_projection_sim3", "sqlm_orb_fuse", "sqlm_orb_search_by_projection_kf",
               "sqlm_orb_search_by_sim3", "sqlm_orb_search_by_bow_kf_frame", "sqlm_orb_search_by_bow_kf_kf", "sqlm_orb_search_for_triangulation",
               "sqlm_orb_bench_extract",
               # DBoW2 vocabulary: BoW transform and batched L1 score
               "sqlm_voc_create", "sqlm_voc_destroy", "sqlm_voc_info", "sqlm_bow_transform", "sqlm_bow_score",
               # LocalMapping: triangulation of new map points and the map-point refresh
               "sqlm_triangulate_pairs", "sqlm_triangulate_pairs_host", "sqlm_triangulate_info",
               "sqlm_map_points_update", "sqlm_map_points_update_host", "sqlm_map_points_update_info"]


class SqlmError(RuntimeError):
    def __init__(self, status: int, what: str):
        super().__init__(f"{what}: {STATUS.get(status, status)} ({status})")
        self.status = status


class Stats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int), ("trials", C.c_int), ("result", C.c_int), ("n_active_edges", C.c_int),
        ("chi2_begin", C.c_double), ("chi2_end", C.c_double), ("lambda_end", C.c_double),
        ("trace_len", C.c_int), ("trace_chi2", C.c_double * TRACE_MAX),
        ("trace_lambda", C.c_double * TRACE_MAX), ("trace_trials", C.c_int * TRACE_MAX),
        ("ms_total", C.c_double), ("ms_setup", C.c_double), ("ms_linearize", C.c_double),
        ("ms_trials", C.c_double),
    ]

    def as_dict(self) -> dict:
        n = self.trace_len
        return dict(iterations=self.iterations, trials=self.trials, result=self.result,
                    n_active_edges=self.n_active_edges, chi2_begin=self.chi2_begin, chi2_end=self.chi2_end,
                    lambda_end=self.lambda_end, trace_chi2=list(self.trace_chi2[:n]),
                    trace_lambda=list(self.trace_lambda[:n]), trace_trials=list(self.trace_trials[:n]),
                    ms_total=self.ms_total, ms_setup=self.ms_setup, ms_linearize=self.ms_linearize,
                    ms_trials=self.ms_trials)


SIM3_TRACE_MAX = 16


class Sim3Stats(C.Structure):
    """sqlm_sim3_stats: one per problem of a sqlm_sim3_optimize call."""
    _fields_ = [
        ("n_corr", C.c_int), ("n_bad", C.c_int),
        ("iterations", C.c_int * 2), ("trials", C.c_int * 2), ("result", C.c_int * 2),
        ("chi2_begin", C.c_double * 2), ("chi2_end", C.c_double * 2), ("lambda_end", C.c_double * 2),
        ("trace_len", C.c_int * 2),
        ("trace_chi2", (C.c_double * SIM3_TRACE_MAX) * 2), ("trace_lambda", (C.c_double * SIM3_TRACE_MAX) * 2),
        ("trace_trials", (C.c_int * SIM3_TRACE_MAX) * 2),
    ]

    def as_dict(self) -> dict:
        n = list(self.trace_len)
        return dict(n_corr=self.n_corr, n_bad=self.n_bad, iterations=list(self.iterations), trials=list(self.trials),
                    result=list(self.result), chi2_begin=list(self.chi2_begin), chi2_end=list(self.chi2_end),
                    lambda_end=list(self.lambda_end),
                    trace_chi2=[list(self.trace_chi2[s][:n[s]]) for s in range(2)],
                    trace_lambda=[list(self.trace_lambda[s][:n[s]]) for s in range(2)],
                    trace_trials=[list(self.trace_trials[s][:n[s]]) for s in range(2)])


POSE_STAGES = 5  # rounds 0-3, LiDAR stage
POSE_CHECKS = 5  # the checks after rounds 0-3, the final classification


class PoseStats(C.Structure):
    """sqlm_pose_stats: one per problem of a sqlm_pose_optimize / sqlm_pose_refine_lidar call."""
    _fields_ = [
        ("n_corr", C.c_int), ("rounds", C.c_int), ("n_bad", C.c_int * 4),
        ("n_lidar", C.c_int), ("n_bad_final", C.c_int),
        ("iterations", C.c_int * POSE_STAGES), ("trials", C.c_int * POSE_STAGES), ("result", C.c_int * POSE_STAGES),
        ("active", C.c_int * POSE_STAGES),
        ("chi2_begin", C.c_double * POSE_STAGES), ("chi2_end", C.c_double * POSE_STAGES),
        ("lambda_end", C.c_double * POSE_STAGES),
    ]

    def as_dict(self) -> dict:
        return dict(n_corr=self.n_corr, rounds=self.rounds, n_bad=list(self.n_bad), n_lidar=self.n_lidar,
                    n_bad_final=self.n_bad_final, iterations=list(self.iterations), trials=list(self.trials),
                    result=list(self.result), active=list(self.active), chi2_begin=list(self.chi2_begin),
                    chi2_end=list(self.chi2_end), lambda_end=list(self.lambda_end))


class LidarSet(C.Structure):
    """sqlm_lidar_set: one map / query search of sqlm_set_lidar_from_cloud_sets."""
    _fields_ = [
        ("kind", C.c_int32), ("n_map_clouds", C.c_int32), ("map_off", C.c_void_p), ("map_xyz", C.c_void_p),
        ("map_Twc", C.c_void_p), ("n_query", C.c_int64), ("query_xyz", C.c_void_p), ("query_Twc", C.c_void_p),
        ("query_normal", C.c_void_p), ("info", C.c_double), ("dist_sq_threshold", C.c_double),
    ]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: build it with __graft_entry__.build() "
                              "(make -C sqrtlm-slam_amd/csrc); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.sqlm_version.restype = C.c_char_p
        L.sqlm_status_string.restype = C.c_char_p
        L.sqlm_kernel_timer_name.restype = C.c_char_p
        if hasattr(L, "sqlm_lidar_associate"):  # build() reports a missing export by name
            P = C.c_void_p
            clouds = [C.c_int, P, P, P, C.c_int64, P, P]  # n_map_clouds, map_off, map_xyz, map_Twc, n_query, query_xyz, query_Twc
            L.sqlm_lidar_associate.argtypes = [P] + clouds + [C.c_double, P, P, P, P, P]
            L.sqlm_set_lidar_from_clouds.argtypes = [P, C.c_int32] + clouds + [P, C.c_double, C.c_double, P]
            L.sqlm_lidar_get_exec_info.argtypes = [P, P]
        if hasattr(L, "sqlm_set_lidar_kind"):
            P = C.c_void_p
            L.sqlm_set_lidar_kind.argtypes = [P, P]
            L.sqlm_set_lidar_from_cloud_sets.argtypes = [P, C.c_int32, C.c_int, P, P]
        if hasattr(L, "sqlm_voc_create"):
            P = C.c_void_p
            # device, k, L, scoring, weighting, n_nodes, parent, is_word, desc, weight, out
            L.sqlm_voc_create.argtypes = [C.c_int] * 5 + [C.c_int32, P, P, P, P, P]
            L.sqlm_voc_destroy.argtypes = [P]
            L.sqlm_voc_info.argtypes = [P, P]
            # ctx, voc, n_img, feat_off, desc, levelsup, word, node, bow_off, bow_word, bow_value
            L.sqlm_bow_transform.argtypes = [P, P, C.c_int, P, P, C.c_int, P, P, P, P, P]
            # ctx, nq, q_word, q_value, n_db, db_off, db_word, db_value, score, n_common
            L.sqlm_bow_score.argtypes = [P, C.c_int64, P, P, C.c_int, P, P, P, P, P]
        if hasattr(L, "sqlm_sim3_ransac"):
            P = C.c_void_p
            # ctx, n_prob, intr1, intr2, fix_scale, min_inliers, pair_off, X1c, X2c, max_err1, max_err2, hyp_off,
            # draws, n_inliers, flags, R12, t12, s12, first_return, best
            L.sqlm_sim3_ransac.argtypes = [P, C.c_int] + [P] * 18
            L.sqlm_sim3_ransac_get_inliers.argtypes = [P, C.c_int, C.c_int, P]
            L.sqlm_sim3_ransac_get_hypothesis.argtypes = [P, C.c_int, C.c_int, P, P, P]
            L.sqlm_sim3_ransac_max_its.argtypes = [C.c_int64, C.c_double, C.c_int, C.c_int]
            L.sqlm_sim3_ransac_scan.argtypes = [C.c_int64, P, C.c_int, P, P, P]
            # n_pair, intr1, intr2, fix_scale, X1c, X2c, max_err1, max_err2, draws, idx, R12, t12, s12, T12, T21,
            # mask, n_inliers
            L.sqlm_sim3_ransac_hypothesis_host.argtypes = [C.c_int, P, P, C.c_int] + [P] * 13
        if hasattr(L, "sqlm_pnp_ransac"):
            P = C.c_void_p
            # ctx, n_prob, intr, min_inliers, pair_off, Xw, uv, max_err, hyp_off, draws, n_inliers, flags, R, t,
            # first_return, best, Tcw, n_refined
            L.sqlm_pnp_ransac.argtypes = [P, C.c_int] + [P] * 16
            L.sqlm_pnp_ransac_get_inliers.argtypes = [P, C.c_int, C.c_int, P]
            # ctx, prob, hyp, R, t, mask, n_inliers, ut, eig, betas, rep_err, chosen
            L.sqlm_pnp_ransac_get_refined.argtypes = [P, C.c_int, C.c_int] + [P] * 9
            # ctx, prob, hyp, idx, ut, eig, betas, rep_err, chosen
            L.sqlm_pnp_ransac_get_hypothesis.argtypes = [P, C.c_int, C.c_int] + [P] * 6
            L.sqlm_pnp_ransac_max_its.argtypes = [C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, P]
            # n_hyp, counts, refined, n_refined, min_inliers, flags, first_return, best, n_record
            L.sqlm_pnp_ransac_scan.argtypes = [C.c_int64, P, P, C.c_int64, C.c_int, P, P, P, P]
            # n_pair, intr, Xw, uv, max_err, draws | in_mask, sweeps, [idx,] R, t, mask, n_inliers, ut, eig, betas,
            # rep_err, chosen
            L.sqlm_pnp_ransac_hypothesis_host.argtypes = [C.c_int] + [P] * 16
            L.sqlm_pnp_ransac_refine_host.argtypes = [C.c_int] + [P] * 15
        if hasattr(L, "sqlm_lidar_features"):
            P = C.c_void_p
            L.sqlm_lidar_features.argtypes = [P, C.c_int] + [P] * 11
            L.sqlm_lidar_features_host.argtypes = [C.c_int] + [P] * 12
            L.sqlm_lidar_features_get_state.argtypes = [P, P]
            L.sqlm_lidar_features_info.argtypes = [P, P]
            L.sqlm_lidar_feat_trig_probe.argtypes = [C.c_int64, P, P, P]
        if hasattr(L, "sqlm_lidar_features_all"):
            P = C.c_void_p
            # ctx, n_sweep, sweep_off, xyz, params, corner, extrinsic, 7 flat outputs, 6 corner outputs
            L.sqlm_lidar_features_all.argtypes = [P, C.c_int] + [P] * 18
            L.sqlm_lidar_features_all_host.argtypes = [C.c_int] + [P] * 20
            L.sqlm_lidar_features_all_get_state.argtypes = [P, P, P]
            L.sqlm_lidar_features_all_info.argtypes = [P, P]
            L.sqlm_lidar_corner_trig_probe.argtypes = [C.c_int64, C.c_int, P, P]
            L.sqlm_lidar_corner_angle_probe.argtypes = [C.c_int64, P, P, P]
        if hasattr(L, "sqlm_lidar_depth"):
            P = C.c_void_p
            # [ctx,] n_frame, sweep_off, xyz, key_off, key_xy, key_un_xy, rows, cols, intrinsic, extrinsic, cam,
            # class_id, depth, nearest_uv, xyz_cam, stats, depth_image [, pixel, winner]
            L.sqlm_lidar_depth.argtypes = [P, C.c_int] + [P] * 5 + [C.c_int, C.c_int] + [P] * 9
            L.sqlm_lidar_depth_host.argtypes = [C.c_int] + [P] * 5 + [C.c_int, C.c_int] + [P] * 11
            L.sqlm_lidar_depth_get_state.argtypes = [P, P, P, P]
            L.sqlm_lidar_depth_info.argtypes = [P, P]
        if hasattr(L, "sqlm_triangulate_pairs"):
            P = C.c_void_p
            # [ctx,] n_pair, pairs, match_off, matches, [sweeps,] x3d, reason, n_new
            L.sqlm_triangulate_pairs.argtypes = [P, C.c_int] + [P] * 6
            L.sqlm_triangulate_pairs_host.argtypes = [C.c_int, P, P, P, C.c_int, P, P, P]
            L.sqlm_triangulate_info.argtypes = [P]
            # [ctx,] n_pt, obs_off, obs_desc, obs_center, pos, ref_center, level_scale, max_scale, best_idx,
            # best_median, normal, max_dist, min_dist
            L.sqlm_map_points_update.argtypes = [P, C.c_int] + [P] * 12
            L.sqlm_map_points_update_host.argtypes = [C.c_int] + [P] * 12
            L.sqlm_map_points_update_info.argtypes = [P, P]
        _lib = L
    return _lib


LF_MAX_ROWS = 128


class LidarFeatParams(C.Structure):
    """sqlm_lidar_feat_params."""
    _fields_ = [("row_num", C.c_int32), ("col_num", C.c_int32), ("num_scan_subregions", C.c_int32),
                ("num_curvature_regions_flat", C.c_int32), ("num_curvature_regions_corner", C.c_int32),
                ("max_surf_flat", C.c_int32), ("max_surf_less_flat", C.c_int32), ("using_sharp_point", C.c_int32),
                ("surf_curv_th", C.c_double), ("max_sq_dis", C.c_double), ("deg_diff", C.c_double),
                ("ring_enabled", C.c_uint8 * LF_MAX_ROWS)]


class LidarFeatState(C.Structure):
    """sqlm_lidar_feat_state: caller-allocated arrays, any may be NULL."""
    _fields_ = [(k, C.c_void_p) for k in ("ring", "scan_off", "scan_src", "scan_col", "image_index", "mask",
                                          "curvature", "neighbours", "sorted", "reason")]


class LidarCornerParams(C.Structure):
    """sqlm_lidar_corner_params."""
    _fields_ = [("max_corner_sharp", C.c_int32), ("max_corner_less_sharp", C.c_int32), ("sharp_curv_th", C.c_double),
                ("ground_z_bound", C.c_double), ("corner_ring_enabled", C.c_uint8 * LF_MAX_ROWS)]


class LidarCornerState(C.Structure):
    """sqlm_lidar_corner_state: caller-allocated arrays, any may be NULL."""
    _fields_ = [(k, C.c_void_p) for k in ("cell_state", "mask", "curvature", "sorted", "reason", "edge", "angle")]


def check(status: int, what: str) -> None:
    if status != SQLM_OK:
        raise SqlmError(status, what)


# int (*sqlm_allreduce_fn)(void *user, void *buf, int64_t count, int dtype, int op)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int)
# int (*sqlm_p2p_fn)(void *user, void *buf, int64_t count, int dtype, int peer, int op)
P2P_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int)
DTYPES = {0: np.float64, 1: np.uint8, 2: np.int32}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)
