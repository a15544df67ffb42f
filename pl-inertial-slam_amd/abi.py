"""ctypes description of the C ABI declared in include/plba.h.

The same signature table binds two different shared objects:
  * the product:  pl-inertial-slam_amd/libplba_hip.so   (prefix ``plba_``), HIP kernels for gfx950;
  * the checker:  oracle/_build/libplba_oracle.so        (prefix ``orc_``), loaded ONLY by tests/,
    __graft_entry__.smoke() and bench.py's cpu_baseline leg (see oracle/oracle.py).
Nothing in this file computes anything: it is the Python spelling of plba.h.
"""
import ctypes as C
import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)

EDGE_POINT, EDGE_LINE, EDGE_IMU_PVR, EDGE_IMU_BIAS, EDGE_PRIOR = range(5)

STATUS = {0: "PLBA_OK", -1: "PLBA_ERR_INVALID", -2: "PLBA_ERR_STATE", -3: "PLBA_ERR_DEVICE",
          -4: "PLBA_ERR_NUMERIC", -5: "PLBA_ERR_EXCHANGE", -6: "PLBA_ERR_INTERNAL"}


class Options(C.Structure):
    _fields_ = [("tau", C.c_double), ("good_step_lower", C.c_double), ("good_step_upper", C.c_double),
                ("max_trials", C.c_int), ("user_lambda_init", C.c_double), ("marg_eps", C.c_double),
                ("fix_line_position_jacobian", C.c_int),
                ("device", C.c_int), ("use_mfma", C.c_int), ("profile", C.c_int), ("factor_block", C.c_int), ("factor_flow", C.c_int), ("chain_elim", C.c_int), ("wide_steps", C.c_int), ("band_solve", C.c_int), ("marg_exact", C.c_int), ("lm_fused", C.c_int),
                ("lm_fused_min_obs", C.c_int), ("lm_group_steps", C.c_int), ("chain_seg", C.c_int), ("twin_max_tiles", C.c_int), ("diag", C.c_int),
                ("pgo_solver", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("trials", C.c_int), ("stop_reason", C.c_int),
                ("solver_failures", C.c_int), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
                ("lambda_final", C.c_double), ("ms_total", C.c_double), ("ms_phase", C.c_double * 8)]


class TraceRow(C.Structure):
    _fields_ = [("iteration", C.c_int), ("trial", C.c_int), ("accepted", C.c_int), ("solver_ok", C.c_int),
                ("lam", C.c_double), ("chi2_current", C.c_double), ("chi2_trial", C.c_double),
                ("scale", C.c_double), ("rho", C.c_double)]


class Prior(C.Structure):
    _fields_ = [("n", C.c_int), ("m", C.c_int), ("nv", C.c_int),
                ("vid", c_int32_p), ("size", c_int32_p), ("idx", c_int32_p),
                ("x0", c_double_p), ("J0", c_double_p), ("r0", c_double_p),
                ("Ar", c_double_p), ("br", c_double_p)]


class LbaOptions(C.Structure):
    _fields_ = [("lambda_lm", C.c_double), ("lambda_k", C.c_double), ("max_iters", C.c_int), ("homog_th", C.c_double),
                ("min_error", C.c_double), ("min_error_change", C.c_double), ("use_iterate_poses", C.c_int), ("variant", C.c_int),
                ("solver", C.c_int)]


class LbaStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("updates", C.c_int), ("err_first", C.c_double), ("err_last", C.c_double),
                ("lam", C.c_double), ("solver_failed", C.c_int), ("reserved", C.c_int)]


class Marginals(C.Structure):
    """plba_marginals of include/plba.h"""
    _fields_ = [("want", C.c_int), ("n_pairs", C.c_int), ("pairs", c_int32_p), ("kf_cov", c_double_p), ("pair_cov", c_double_p),
                ("pt_cov", c_double_p), ("pt_status", c_uint8_p), ("ln_cov", c_double_p), ("ln_status", c_uint8_p),
                ("n_excluded", C.c_int32 * 2)]


class Slide(C.Structure):
    """plba_slide of include/plba.h"""
    _fields_ = [("n_drop", C.c_int), ("drop_point", c_uint8_p), ("drop_line", c_uint8_p), ("drop_point_obs", c_uint8_p), ("drop_line_obs", c_uint8_p),
                ("K_add", C.c_int), ("vid_pvr", c_int32_p), ("vid_bias", c_int32_p),
                ("P3", c_double_p), ("V3", c_double_p), ("q_xyzw4", c_double_p), ("bg3", c_double_p), ("ba3", c_double_p), ("dbg3", c_double_p), ("dba3", c_double_p),
                ("fixed_pvr", c_uint8_p), ("fixed_bias", c_uint8_p),
                ("M_add", C.c_int), ("imu_kf_i", c_int32_p), ("imu_kf_j", c_int32_p), ("preint142", c_double_p), ("info_pvr81", c_double_p), ("info_bias36", c_double_p),
                ("Np_add", C.c_int), ("xyz3", c_double_p), ("point_fixed", c_uint8_p),
                ("Nl_add", C.c_int), ("sPeP6", c_double_p), ("line_fixed", c_uint8_p),
                ("Ep_add", C.c_int), ("po_pt", c_int32_p), ("po_kf", c_int32_p), ("uv2", c_double_p), ("po_inv_sigma2", c_double_p),
                ("El_add", C.c_int), ("lo_ln", c_int32_p), ("lo_kf", c_int32_p), ("l3", c_double_p), ("lo_inv_sigma2", c_double_p)]


class PoseGraph(C.Structure):
    """plba_pose_graph of include/plba.h"""
    _fields_ = [("nv", C.c_int), ("pose12", c_double_p), ("fixed", c_uint8_p), ("ne", C.c_int), ("ei", c_int32_p), ("ej", c_int32_p),
                ("meas12", c_double_p), ("info36", c_double_p)]


class PgoMarginals(C.Structure):
    """plba_pgo_marginals of include/plba.h"""
    _fields_ = [("want", C.c_int), ("n_pairs", C.c_int), ("pairs", c_int32_p), ("v_cov", c_double_p), ("v_status", c_uint8_p),
                ("pair_cov", c_double_p), ("pair_status", c_uint8_p), ("n_status", C.c_int32 * 4)]


class RefineOptions(C.Structure):
    """plba_refine_options of include/plba.h"""
    _fields_ = [("max_iters", C.c_int), ("max_trials", C.c_int), ("lambda_init", C.c_double), ("select_point", c_uint8_p), ("select_line", c_uint8_p),
                ("status", c_uint8_p), ("iters", c_int32_p), ("trials", c_int32_p)]


class RefineStats(C.Structure):
    """plba_refine_stats of include/plba.h"""
    _fields_ = [("n_refined", C.c_int), ("n_skipped", C.c_int), ("n_exhausted", C.c_int), ("iterations", C.c_longlong), ("trials", C.c_longlong),
                ("chi2_before", C.c_double), ("chi2_after", C.c_double), ("ms_total", C.c_double)]


class RelposeOptions(C.Structure):
    """plba_relpose_options of include/plba.h"""
    _fields_ = [("max_iters", C.c_int), ("max_iters_ref", C.c_int), ("homog_th", C.c_double), ("chi2_th", C.c_double), ("protocol", C.c_int),
                ("reserved", C.c_int), ("lc_res", C.c_double), ("lc_unc", C.c_double), ("lc_inl", C.c_double), ("lc_trs", C.c_double), ("lc_rot", C.c_double)]


class RelposeResult(C.Structure):
    """plba_relpose_result of include/plba.h"""
    _fields_ = [("T_inc16", C.c_double * 16), ("pose_inc6", C.c_double * 6), ("H36", C.c_double * 36), ("e", C.c_double), ("cov_eig6", C.c_double * 6),
                ("t", C.c_double), ("r", C.c_double), ("n_inliers", C.c_int32), ("iters", C.c_int32 * 2), ("status", C.c_int32), ("accepted", C.c_int32),
                ("lc_res", C.c_int32), ("lc_unc", C.c_int32), ("lc_inl", C.c_int32), ("lc_trs", C.c_int32), ("lc_rot", C.c_int32)]


class TrackOptions(C.Structure):
    """plba_track_options of include/plba.h"""
    _fields_ = [("max_iters", C.c_int), ("max_iters_ref", C.c_int), ("min_features", C.c_int), ("reserved", C.c_int), ("homog_th", C.c_double),
                ("min_error", C.c_double), ("min_error_change", C.c_double), ("inlier_k", C.c_double)]


class TrackResult(C.Structure):
    """plba_track_result of include/plba.h"""
    _fields_ = [("DT16", C.c_double * 16), ("T_opt16", C.c_double * 16), ("H36", C.c_double * 36), ("cov36", C.c_double * 36), ("cov_eig6", C.c_double * 6),
                ("err", C.c_double), ("pt_mean", C.c_double), ("pt_stdv", C.c_double), ("ln_mean", C.c_double), ("ln_stdv", C.c_double),
                ("n_inliers_pt", C.c_int32), ("n_inliers_ln", C.c_int32), ("iters", C.c_int32 * 3), ("path", C.c_int32), ("status", C.c_int32), ("good", C.c_int32)]


class VitrackOptions(C.Structure):
    """plba_vitrack_options of include/plba.h"""
    _fields_ = [("rounds", C.c_int), ("iters", C.c_int), ("max_trials", C.c_int), ("robust_rounds", C.c_int), ("tau", C.c_double), ("user_lambda_init", C.c_double),
                ("huber_pt", C.c_double), ("huber_ln", C.c_double), ("huber_imu", C.c_double), ("chi2_pt", C.c_double), ("chi2_ln", C.c_double)]


class VitrackResult(C.Structure):
    """plba_vitrack_result of include/plba.h"""
    _fields_ = [("state_i22", C.c_double * 22), ("state_j22", C.c_double * 22), ("H900", C.c_double * 900), ("next_prior_info225", C.c_double * 225),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double), ("iterations", C.c_int32 * 8), ("stop_reason", C.c_int32 * 8),
                ("trials", C.c_int32), ("solver_failures", C.c_int32), ("n_inliers_pt", C.c_int32), ("n_inliers_ln", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


class MatchOptions(C.Structure):
    """plba_match_options of include/plba.h"""
    _fields_ = [("nnr", C.c_float), ("best_lr", C.c_int)]


class LoopOptions(C.Structure):
    """plba_loop_options of include/plba.h"""
    _fields_ = [("match_pt", MatchOptions), ("match_ln", MatchOptions), ("use_points", C.c_int), ("use_lines", C.c_int), ("lc_inlier_ratio", C.c_double),
                ("relpose", RelposeOptions)]


class LoopResult(C.Structure):
    """plba_loop_result of include/plba.h"""
    _fields_ = [("common_pt", C.c_int32), ("common_ls", C.c_int32), ("ratio_ok", C.c_int32), ("reserved", C.c_int32), ("inl_ratio_pt", C.c_double),
                ("inl_ratio_ls", C.c_double), ("relpose", RelposeResult)]


class BowOptions(C.Structure):
    """plba_bow_options of include/plba.h"""
    _fields_ = [("mode", C.c_int32), ("topk", C.c_int32), ("lc_kf_dist", C.c_int32), ("lc_kf_max_dist", C.c_int32), ("lc_nkf_closest", C.c_int32),
                ("min_lm_cov_graph", C.c_int32), ("min_kf_local_map", C.c_int32), ("reserved", C.c_int32)]


class BowCandidate(C.Structure):
    """plba_bow_candidate of include/plba.h"""
    _fields_ = [("is_candidate", C.c_int32), ("kf_prev", C.c_int32), ("n_closest", C.c_int32), ("n_eligible", C.c_int32), ("best_score", C.c_double),
                ("lc_min_score", C.c_double), ("topk", C.c_int32 * 16), ("topk_score", C.c_double * 16)]


class BowResult(C.Structure):
    """plba_bow_result of include/plba.h"""
    _fields_ = [("first_index", C.c_int32), ("reserved", C.c_int32), ("score_cap", C.c_int64), ("score_p", c_double_p), ("score_l", c_double_p),
                ("score", c_double_p), ("score_f32", C.POINTER(C.c_float)), ("pt_word", c_int32_p), ("pt_bow_id", c_int32_p), ("pt_bow_val", c_double_p),
                ("pt_nnz", c_int32_p), ("ln_word", c_int32_p), ("ln_bow_id", c_int32_p), ("ln_bow_val", c_double_p), ("ln_nnz", c_int32_p),
                ("cand", C.POINTER(BowCandidate))]


class CovisOptions(C.Structure):
    """plba_covis_options of include/plba.h"""
    _fields_ = [("min_lm_ess_graph", C.c_int32), ("min_lm_cov_graph", C.c_int32), ("min_kf_local_map", C.c_int32), ("reserved", C.c_int32)]


BOW_COMBINED, BOW_POINTS, BOW_LINES = range(3)
RELPOSE_OK, RELPOSE_EMPTY, RELPOSE_NONFINITE, RELPOSE_RANK = range(4)
TRACK_OK, TRACK_NONFINITE, TRACK_RANK = 0, 2, 3
TRACK_REFINED, TRACK_ROBUST, TRACK_FEW_BEFORE, TRACK_FEW_AFTER = range(4)
VITRACK_OK, VITRACK_NONFINITE, VITRACK_SINGULAR = 0, 2, 3
# VitrackResult as a numpy record, for reading an array of them at once
VITRACK_RESULT_DT = np.dtype([("state_i22", np.float64, 22), ("state_j22", np.float64, 22), ("H900", np.float64, (30, 30)), ("next_prior_info225", np.float64, (15, 15)),
                              ("chi2_initial", np.float64), ("chi2_final", np.float64), ("lambda_final", np.float64), ("iterations", np.int32, 8), ("stop_reason", np.int32, 8),
                              ("trials", np.int32), ("solver_failures", np.int32), ("n_inliers_pt", np.int32), ("n_inliers_ln", np.int32), ("status", np.int32), ("reserved", np.int32)])
assert VITRACK_RESULT_DT.itemsize == C.sizeof(VitrackResult)
REFINE_DONE, REFINE_EXHAUSTED, REFINE_NONFINITE, REFINE_FIXED, REFINE_UNSELECTED, REFINE_NO_OBS = range(6)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)

_P = C.c_void_p  # plba_problem*

# entry points of the product that have no counterpart in the reference's algorithm (memory management of the device-resident window): the
# CPU oracle — a restatement of the reference — does not implement them
# (compute_marginals: the reference computes no marginals; the oracle has no such entry.  optimize_pose_graph: the oracle restates the
# pose graph as orc_pgo, a checker entry of its own outside this table.  refine_landmarks: g2o's structure-only solver is a stub at the
# reference's boundary; its checker is the numpy restatement tests/refine_ref.py.  relative_pose: its checker is tests/relpose_ref.py.
# track_pose: its checker is tests/track_ref.py.  match_descriptors, verify_loop_candidates: their checker is tests/match_ref.py.
# bow_*: their checker is tests/bow_ref.py.  pose_graph_marginals: the reference computes none; its checker is tests/pgo_cov_ref.py.
# track_inertial: the reference never instantiates the graph; its checker is tests/vitrack_ref.py.  covis_*: their checker is
# tests/covis_ref.py)
PRODUCT_ONLY = {"slide_window", "get_sizes", "marginalize_to_prior", "get_prior", "compute_marginals", "optimize_pose_graph",
                "pose_graph_marginals",
                "refine_default_options", "refine_landmarks", "relpose_default_options", "relative_pose", "track_default_options", "track_pose",
                "vitrack_default_options", "track_inertial",
                "match_default_options", "match_descriptors", "loop_default_options", "verify_loop_candidates",
                "bow_default_options", "bow_set_vocabulary", "bow_transform", "bow_insert_keyframes", "bow_remove_keyframe", "bow_reset",
                "covis_default_options", "covis_set_map", "covis_reset", "covis_rows", "covis_column", "covis_pose_graph", "covis_local_map"}

# name -> (restype, argtypes); every symbol plba.h declares
SIGNATURES = {
    "default_options": (None, [C.POINTER(Options)]),
    "create": (C.c_int, [C.POINTER(Options), C.POINTER(_P)]),
    "destroy": (None, [_P]),
    "last_error": (C.c_char_p, [_P]),
    "backend_name": (C.c_char_p, []),
    "set_camera": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_double, c_double_p, c_double_p]),
    "set_gravity": (C.c_int, [_P, c_double_p]),
    "set_keyframes": (C.c_int, [_P, C.c_int, c_int32_p, c_int32_p] + [c_double_p] * 7 + [c_uint8_p, c_uint8_p]),
    "set_points": (C.c_int, [_P, C.c_int, c_double_p, c_uint8_p]),
    "set_lines": (C.c_int, [_P, C.c_int, c_double_p, c_uint8_p]),
    "set_point_obs": (C.c_int, [_P, C.c_int, c_int32_p, c_int32_p, c_double_p, c_double_p]),
    "set_line_obs": (C.c_int, [_P, C.c_int, c_int32_p, c_int32_p, c_double_p, c_double_p]),
    "set_imu_edges": (C.c_int, [_P, C.c_int, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    "set_prior": (C.c_int, [_P, C.c_int, C.c_int, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    "set_robust": (C.c_int, [_P, C.c_int, C.c_int, C.c_double]),
    "set_levels": (C.c_int, [_P, C.c_int, c_uint8_p]),
    "get_levels": (C.c_int, [_P, C.c_int, c_uint8_p]),
    "slide_window": (C.c_int, [_P, C.POINTER(Slide), c_int32_p, c_int32_p]),
    "get_sizes": (C.c_int, [_P, c_int32_p]),
    "set_shard": (C.c_int, [_P, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]),
    "set_stream": (C.c_int, [_P, C.c_void_p]),
    "optimize": (C.c_int, [_P, C.c_int, c_uint8_p, C.POINTER(Stats)]),
    "gate_outliers": (C.c_int, [_P, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "recompute_errors": (C.c_int, [_P]),
    "cull_observations": (C.c_int, [_P, C.c_double, c_uint8_p, c_uint8_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "get_edge_chi2": (C.c_int, [_P, C.c_int, c_double_p, c_uint8_p]),
    "get_trace": (C.c_int, [_P, C.POINTER(TraceRow), C.c_int, C.POINTER(C.c_int)]),
    "get_keyframes": (C.c_int, [_P] + [c_double_p] * 5),
    "get_points": (C.c_int, [_P, c_double_p]),
    "get_lines": (C.c_int, [_P, c_double_p]),
    "save_state": (C.c_int, [_P]),
    "restore_state": (C.c_int, [_P]),
    "marginalize": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(Prior)]),
    "marginalize_factors": (C.c_int, [_P, C.c_int, c_int32_p, C.c_int, c_int32_p, C.c_int, c_int32_p, C.c_int, C.c_int, c_int32_p, C.POINTER(Prior)]),
    "preintegrate": (C.c_int, [_P, C.c_int, c_int32_p, C.POINTER(C.c_longdouble), c_double_p, c_double_p, C.POINTER(C.c_longdouble), C.POINTER(C.c_longdouble), c_double_p, c_double_p, C.c_double, C.c_double, c_double_p]),
    "marginalize_to_prior": (C.c_int, [_P, C.c_int, C.c_int, c_int32_p]),
    "get_prior": (C.c_int, [_P, C.POINTER(Prior)]),
    "prior_free": (None, [C.POINTER(Prior)]),
    "compute_marginals": (C.c_int, [_P, C.POINTER(Marginals)]),
    "set_marg_eps": (C.c_int, [_P, C.c_double]),
    "lba_default_options": (None, [C.POINTER(LbaOptions)]),
    "lba_visual": (C.c_int, [_P, C.POINTER(LbaOptions), C.c_int, c_double_p, c_int32_p, C.c_int, c_double_p, C.c_int, c_double_p,
                             C.c_int, c_int32_p, c_int32_p, c_double_p, C.c_int, c_int32_p, c_int32_p, c_double_p,
                             C.c_double, C.c_double, C.c_double, C.c_double, c_double_p, c_uint8_p, c_uint8_p, C.POINTER(LbaStats)]),
    "debug_build": (C.c_int, [_P, C.c_double, C.c_int]),
    "debug_get": (C.c_int, [_P, C.c_char_p, c_double_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dense_solve": (C.c_int, [_P, C.c_int, c_double_p, c_double_p, c_double_p, C.POINTER(C.c_int)]),
    "debug_dense_solve": (C.c_int, [_P, C.c_int, c_double_p, c_double_p, c_double_p, C.POINTER(C.c_int)]),
    "refine_default_options": (None, [C.POINTER(RefineOptions)]),
    "refine_landmarks": (C.c_int, [_P, C.POINTER(RefineOptions), C.POINTER(RefineStats)]),
    "relpose_default_options": (None, [C.POINTER(RelposeOptions)]),
    "relative_pose": (C.c_int, [_P, C.POINTER(RelposeOptions), C.c_int, c_int32_p, c_double_p, c_double_p, c_int32_p, c_double_p, c_double_p,
                                C.c_double, C.c_double, C.c_double, C.c_double, c_double_p, c_uint8_p, c_uint8_p, C.POINTER(RelposeResult)]),
    "track_default_options": (None, [C.POINTER(TrackOptions)]),
    "track_pose": (C.c_int, [_P, C.POINTER(TrackOptions), C.c_int, c_int32_p, c_double_p, c_double_p, c_double_p, c_int32_p, c_double_p, c_double_p,
                             c_double_p, c_double_p, C.c_double, C.c_double, C.c_double, C.c_double, c_double_p, c_uint8_p, c_uint8_p, C.POINTER(TrackResult)]),
    "vitrack_default_options": (None, [C.POINTER(VitrackOptions)]),
    "track_inertial": (C.c_int, [_P, C.POINTER(VitrackOptions), C.c_int, c_uint8_p] + [c_double_p] * 8 + [c_int32_p, c_double_p, c_double_p, c_double_p, c_int32_p, c_double_p,
                                 c_double_p, c_double_p, C.c_double, C.c_double, C.c_double, C.c_double, c_double_p, c_double_p, c_uint8_p, c_uint8_p, C.POINTER(VitrackResult)]),
    "match_default_options": (None, [C.POINTER(MatchOptions)]),
    "match_descriptors": (C.c_int, [_P, C.POINTER(MatchOptions), C.c_int, c_int32_p, c_uint8_p, c_int32_p, c_uint8_p, C.POINTER(C.c_float), c_int32_p, c_int32_p,
                                    c_int32_p]),
    "loop_default_options": (None, [C.POINTER(LoopOptions)]),
    "verify_loop_candidates": (C.c_int, [_P, C.POINTER(LoopOptions), C.c_int, c_int32_p, c_uint8_p, c_double_p, c_int32_p, c_uint8_p, c_double_p,
                                         c_int32_p, c_uint8_p, c_double_p, c_int32_p, c_uint8_p, c_double_p, C.c_double, C.c_double, C.c_double, C.c_double,
                                         c_int32_p, c_int32_p, c_uint8_p, c_uint8_p, C.POINTER(LoopResult)]),
    "bow_default_options": (None, [C.POINTER(BowOptions)]),
    "bow_set_vocabulary": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, c_uint8_p, c_double_p, c_int32_p]),
    "bow_transform": (C.c_int, [_P, C.c_int, C.c_int, c_int32_p, c_uint8_p, c_int32_p, c_int32_p, c_double_p, c_int32_p]),
    "bow_insert_keyframes": (C.c_int, [_P, C.POINTER(BowOptions), C.c_int, c_int32_p, c_uint8_p, c_double_p, c_int32_p, c_uint8_p, c_double_p, c_int32_p,
                                       c_int32_p, C.POINTER(BowResult)]),
    "bow_remove_keyframe": (C.c_int, [_P, C.c_int]),
    "bow_reset": (C.c_int, [_P]),
    "covis_default_options": (None, [C.POINTER(CovisOptions)]),
    "covis_set_map": (C.c_int, [_P, C.c_int, c_uint8_p, C.c_int, c_int32_p, c_int32_p, C.c_int, c_int32_p, c_int32_p, c_double_p]),
    "covis_reset": (C.c_int, [_P]),
    "covis_rows": (C.c_int, [_P, C.c_int, c_int32_p, C.c_int, c_int32_p, C.c_int, c_int32_p, c_int32_p]),
    "covis_column": (C.c_int, [_P, C.c_int, c_int32_p]),
    "covis_pose_graph": (C.c_int, [_P, C.POINTER(CovisOptions), C.c_int, c_double_p, C.c_int, c_int32_p, c_double_p, C.c_int, c_int32_p, c_int32_p, c_double_p,
                                   C.POINTER(C.c_int)]),
    "covis_local_map": (C.c_int, [_P, C.POINTER(CovisOptions), C.c_int, c_uint8_p, c_uint8_p, c_uint8_p, c_int32_p]),
    "optimize_pose_graph": (C.c_int, [_P, C.POINTER(PoseGraph), C.c_int, C.c_double, C.c_int, C.POINTER(Stats), C.POINTER(TraceRow), C.c_int, C.POINTER(C.c_int)]),
    "pose_graph_marginals": (C.c_int, [_P, C.POINTER(PoseGraph), C.POINTER(PgoMarginals)]),
}


class PlbaError(RuntimeError):
    pass


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


def _ip(a):
    return None if a is None else a.ctypes.data_as(c_int32_p)


def _up(a):
    return None if a is None else a.ctypes.data_as(c_uint8_p)


def _f64(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)


def _desc_csr(lists):
    """(start, rows) of a list of (n, 32) uint8 descriptor arrays; None or an empty array is an empty side"""
    arrs = [np.zeros((0, 32), np.uint8) if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32) for a in lists]
    start = np.zeros(len(arrs) + 1, np.int32)
    start[1:] = np.cumsum([len(a) for a in arrs])
    return start, (np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros((0, 32), np.uint8))


def _relpose_dict(res):
    """a list of RelposeResult as arrays over the candidates"""
    B = len(res)
    out = dict(T_inc=np.array([list(r.T_inc16) for r in res]).reshape(B, 4, 4), pose_inc=np.array([list(r.pose_inc6) for r in res]).reshape(B, 6),
               H=np.array([list(r.H36) for r in res]).reshape(B, 6, 6), cov_eig=np.array([list(r.cov_eig6) for r in res]).reshape(B, 6),
               iters=np.array([list(r.iters) for r in res], np.int32).reshape(B, 2))
    for k in ("e", "t", "r"):
        out[k] = np.array([getattr(r, k) for r in res], np.float64)
    for k in ("n_inliers", "status", "accepted", "lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot"):
        out[k] = np.array([getattr(r, k) for r in res], np.int32)
    return out


class Lib:
    """A loaded implementation of plba.h (``prefix`` selects plba_* or orc_*)."""

    def __init__(self, path, prefix, optional=False):
        self.path = str(path)
        self.prefix = prefix
        self.cdll = C.CDLL(self.path)
        self.fn = {}
        missing = []
        for name, (res, args) in SIGNATURES.items():
            sym = prefix + name
            try:
                f = getattr(self.cdll, sym)
            except AttributeError:
                missing.append(sym)
                continue
            f.restype = res
            f.argtypes = args
            self.fn[name] = f
        missing = [m for m in missing if not (prefix != "plba_" and m[len(prefix):] in PRODUCT_ONLY)]
        if missing and not optional:      # (optional: a library that implements a subset — the quad-precision oracle build, oracle/make_quad.py)
            raise PlbaError("%s does not export: %s" % (self.path, ", ".join(missing)))

    def backend_name(self):
        return self.fn["backend_name"]().decode()

    def default_options(self):
        o = Options()
        self.fn["default_options"](C.byref(o))
        return o


def make_slide(d):
    """The plba_slide of include/plba.h for `d` as window.slide_delta() makes it; returns (struct, arrays its pointers refer to)."""
    keep = []

    def f64(a, shape=None):
        if a is None:
            return None
        a = _f64(a, shape); keep.append(a); return _dp(a)

    def i32(a):
        if a is None:
            return None
        a = _i32(a); keep.append(a); return _ip(a)

    def u8(a):
        if a is None:
            return None
        a = _u8(a); keep.append(a); return _up(a)
    s = Slide()
    s.n_drop = int(d.get("n_drop", 0))
    s.drop_point, s.drop_line = u8(d.get("drop_point")), u8(d.get("drop_line"))
    s.drop_point_obs, s.drop_line_obs = u8(d.get("drop_point_obs")), u8(d.get("drop_line_obs"))
    k = d.get("kf")
    s.K_add = 0 if k is None else len(k["vid_pvr"])
    if k is not None:
        s.vid_pvr, s.vid_bias = i32(k["vid_pvr"]), i32(k.get("vid_bias"))
        s.P3, s.V3, s.q_xyzw4 = f64(k["P"]), f64(k["V"]), f64(k["q"])
        s.bg3, s.ba3, s.dbg3, s.dba3 = f64(k.get("bg")), f64(k.get("ba")), f64(k.get("dbg")), f64(k.get("dba"))
    s.fixed_pvr, s.fixed_bias = u8(d.get("fixed_pvr")), u8(d.get("fixed_bias"))
    im = d.get("imu")
    s.M_add = 0 if im is None else len(im["kf_i"])
    if im is not None:
        s.imu_kf_i, s.imu_kf_j = i32(im["kf_i"]), i32(im["kf_j"])
        s.preint142, s.info_pvr81, s.info_bias36 = f64(im["preint"], (-1, 142)), f64(im["info_pvr"], (-1, 81)), f64(im["info_bias"], (-1, 36))
    pts, lns = d.get("points"), d.get("lines")
    s.Np_add = 0 if pts is None else len(pts); s.xyz3 = f64(pts, (-1, 3)) if s.Np_add else None; s.point_fixed = u8(d.get("point_fixed"))
    s.Nl_add = 0 if lns is None else len(lns); s.sPeP6 = f64(lns, (-1, 6)) if s.Nl_add else None; s.line_fixed = u8(d.get("line_fixed"))
    s.Ep_add = len(d["po_pt"]) if d.get("po_pt") is not None else 0
    if s.Ep_add:
        s.po_pt, s.po_kf, s.uv2, s.po_inv_sigma2 = i32(d["po_pt"]), i32(d["po_kf"]), f64(d["po_uv"], (-1, 2)), f64(d.get("po_w"))
    s.El_add = len(d["lo_ln"]) if d.get("lo_ln") is not None else 0
    if s.El_add:
        s.lo_ln, s.lo_kf, s.l3, s.lo_inv_sigma2 = i32(d["lo_ln"]), i32(d["lo_kf"]), f64(d["lo_l"], (-1, 3)), f64(d.get("lo_w"))
    return s, keep


class Problem:
    """One BA problem = one g2o::SparseOptimizer of the reference call site
    (src/mapHandler.cpp:5787-5797), behind the C ABI."""

    def __init__(self, lib, **opts):
        self.lib = lib
        o = lib.default_options()
        for k, v in opts.items():
            if not hasattr(o, k):
                raise PlbaError("unknown option %r" % k)
            setattr(o, k, v)
        self._h = _P()
        rc = lib.fn["create"](C.byref(o), C.byref(self._h))
        if rc != 0:
            msg = lib.fn["last_error"](None)
            raise PlbaError("create failed: %s (%s)" % (STATUS.get(rc, rc), msg.decode() if msg else ""))
        self._cb = None
        self.dims = {}

    # -- plumbing -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.fn["destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, allow_positive=False):
        if rc < 0 or (rc > 0 and not allow_positive):
            msg = self.lib.fn["last_error"](self._h)
            raise PlbaError("%s: %s" % (STATUS.get(rc, rc), msg.decode() if msg else ""))
        return rc

    def call(self, name, *args, allow_positive=False):
        return self._ck(self.lib.fn[name](self._h, *args), allow_positive)

    # -- upload ------------------------------------------------------------------------------
    def set_camera(self, fx, fy, cx, cy, Rbc, Pbc):
        Rbc = _f64(Rbc, (9,)); Pbc = _f64(Pbc, (3,))
        self.call("set_camera", fx, fy, cx, cy, _dp(Rbc), _dp(Pbc))

    def set_gravity(self, gw):
        gw = _f64(gw, (3,))
        self.call("set_gravity", _dp(gw))

    def set_keyframes(self, vid_pvr, vid_bias, P, V, q, bg=None, ba=None, dbg=None, dba=None,
                      fixed_pvr=None, fixed_bias=None):
        K = len(vid_pvr)
        arrs = [_f64(a) for a in (P, V, q, bg, ba, dbg, dba)]
        vp, vb = _i32(vid_pvr), _i32(vid_bias)
        fp, fb = _u8(fixed_pvr), _u8(fixed_bias)
        self.call("set_keyframes", K, _ip(vp), _ip(vb), *[_dp(a) for a in arrs], _up(fp), _up(fb))
        self.dims["K"] = K

    def set_points(self, xyz, fixed=None):
        xyz = _f64(xyz, (-1, 3)); f = _u8(fixed)
        self.call("set_points", len(xyz), _dp(xyz), _up(f))
        self.dims["Np"] = len(xyz)

    def set_lines(self, sPeP, fixed=None):
        l = _f64(sPeP, (-1, 6)); f = _u8(fixed)
        self.call("set_lines", len(l), _dp(l), _up(f))
        self.dims["Nl"] = len(l)

    def set_point_obs(self, pt, kf, uv, inv_sigma2=None):
        pt, kf, uv, w = _i32(pt), _i32(kf), _f64(uv, (-1, 2)), _f64(inv_sigma2)
        self.call("set_point_obs", len(pt), _ip(pt), _ip(kf), _dp(uv), _dp(w))
        self.dims["Ep"] = len(pt)

    def set_line_obs(self, ln, kf, l3, inv_sigma2=None):
        ln, kf, l3, w = _i32(ln), _i32(kf), _f64(l3, (-1, 3)), _f64(inv_sigma2)
        self.call("set_line_obs", len(ln), _ip(ln), _ip(kf), _dp(l3), _dp(w))
        self.dims["El"] = len(ln)

    def set_imu_edges(self, kf_i, kf_j, preint142, info_pvr, info_bias):
        ki, kj = _i32(kf_i), _i32(kf_j)
        pre, ip, ib = _f64(preint142, (-1, 142)), _f64(info_pvr, (-1, 81)), _f64(info_bias, (-1, 36))
        self.call("set_imu_edges", len(ki), _ip(ki), _ip(kj), _dp(pre), _dp(ip), _dp(ib))
        self.dims["M"] = len(ki)

    def set_prior(self, prior):
        """prior: dict(n, vid, size, idx, x0, J0 (n x n, J0[r, c]), r0) or None to clear."""
        if prior is None or len(prior["vid"]) == 0:
            self.call("set_prior", 0, 0, None, None, None, None, None, None)
            self.dims["n_prior"] = 0
            return
        n = int(prior["n"])
        vid, size, idx = _i32(prior["vid"]), _i32(prior["size"]), _i32(prior["idx"])
        x0, r0 = _f64(prior["x0"]), _f64(prior["r0"])
        J0 = np.asfortranarray(np.asarray(prior["J0"], dtype=np.float64).reshape(n, n))  # column-major
        self.call("set_prior", n, len(vid), _ip(vid), _ip(size), _ip(idx), _dp(x0),
                  J0.ctypes.data_as(c_double_p), _dp(r0))
        self.dims["n_prior"] = n

    def set_robust(self, kind, enabled, delta=0.0):
        self.call("set_robust", kind, int(enabled), float(delta))

    def set_levels(self, kind, level):
        lv = _u8(level)
        self.call("set_levels", kind, _up(lv))

    def get_levels(self, kind):
        n = self.dims["Ep"] if kind == EDGE_POINT else self.dims["El"]
        lv = np.zeros(n, np.uint8)
        self.call("get_levels", kind, _up(lv))
        return lv

    def set_shard(self, rank, world, allreduce):
        """allreduce(dev_ptr:int, n:int, op:int, stream:int) -> None, raising on failure."""
        def _tramp(user, buf, n, op, stream):
            try:
                allreduce(buf, n, op, stream)
                return 0
            except Exception as e:  # surfaced as PLBA_ERR_EXCHANGE
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLREDUCE_FN(_tramp)
        self.call("set_shard", rank, world, self._cb, None)

    def set_shard_native(self, rank, world, fn_addr, user_ptr):
        """plba_set_shard with a NATIVE plba_allreduce_fn (e.g. plba_rccl_allreduce of include/plba_rccl.h) and its user
        pointer: no Python frame runs inside the LM loop."""
        self._cb = C.cast(C.c_void_p(fn_addr), ALLREDUCE_FN)
        self.call("set_shard", rank, world, self._cb, C.c_void_p(user_ptr))

    def set_stream(self, stream_handle):
        self.call("set_stream", C.c_void_p(stream_handle))

    # -- solve -------------------------------------------------------------------------------
    def optimize(self, iters, abort=None):
        st = Stats()
        ab = _up(abort) if abort is not None else None
        self.call("optimize", int(iters), ab, C.byref(st))
        return st

    def gate_outliers(self, thresh=5.991):
        a, b = C.c_int(0), C.c_int(0)
        self.call("gate_outliers", float(thresh), C.byref(a), C.byref(b), allow_positive=True)
        return a.value, b.value

    def recompute_errors(self):
        self.call("recompute_errors")

    def cull_observations(self, thresh=5.991):
        """Culling decision of the call site after the final optimize (mapHandler.cpp:5541-5620): per-observation
        bad flags for points and lines (level-1 edges are re-evaluated on the final estimates first)."""
        Ep, El = self.dims.get("Ep", 0), self.dims.get("El", 0)
        bp, bl = np.zeros(max(Ep, 1), np.uint8), np.zeros(max(El, 1), np.uint8)
        a, b = C.c_int(0), C.c_int(0)
        self.call("cull_observations", float(thresh), _up(bp), _up(bl), C.byref(a), C.byref(b), allow_positive=True)
        return {"bad_points": bp[:Ep].astype(bool), "bad_lines": bl[:El].astype(bool), "n_points": a.value, "n_lines": b.value}

    def edge_chi2(self, kind):
        n = {EDGE_POINT: self.dims.get("Ep", 0), EDGE_LINE: self.dims.get("El", 0),
             EDGE_IMU_PVR: self.dims.get("M", 0), EDGE_IMU_BIAS: self.dims.get("M", 0), EDGE_PRIOR: 1}[kind]
        chi = np.zeros(n); dp = np.zeros(n, np.uint8)
        self.call("get_edge_chi2", kind, _dp(chi), _up(dp))
        return chi, dp

    def trace(self):
        n = C.c_int(0)
        self.call("get_trace", None, 0, C.byref(n))
        rows = (TraceRow * max(n.value, 1))()
        self.call("get_trace", rows, n.value, C.byref(n))
        return [dict(iteration=r.iteration, trial=r.trial, accepted=r.accepted, solver_ok=r.solver_ok,
                     lam=r.lam, chi2_current=r.chi2_current, chi2_trial=r.chi2_trial, scale=r.scale, rho=r.rho)
                for r in rows[:n.value]]

    # -- results -----------------------------------------------------------------------------
    def get_keyframes(self):
        K = self.dims["K"]
        P, V, q, dbg, dba = np.zeros((K, 3)), np.zeros((K, 3)), np.zeros((K, 4)), np.zeros((K, 3)), np.zeros((K, 3))
        self.call("get_keyframes", _dp(P), _dp(V), _dp(q), _dp(dbg), _dp(dba))
        return dict(P=P, V=V, q=q, dbg=dbg, dba=dba)

    def get_points(self):
        a = np.zeros((self.dims.get("Np", 0), 3))
        if len(a):
            self.call("get_points", _dp(a))
        return a

    def get_lines(self):
        a = np.zeros((self.dims.get("Nl", 0), 6))
        if len(a):
            self.call("get_lines", _dp(a))
        return a

    def save_state(self):
        self.call("save_state")

    def restore_state(self):
        self.call("restore_state")

    def set_marg_eps(self, eps):
        self.call("set_marg_eps", float(eps))

    def marginalize(self, first_kf=0, max_edges=50):
        pr = Prior()
        self.call("marginalize", int(first_kf), int(max_edges), C.byref(pr))
        return self._prior_dict(pr)

    def marginalize_to_prior(self, first_kf=0, max_edges=50):
        """plba_marginalize_to_prior: the marginalization's result becomes this problem's prior on the device (nothing comes back);
        returns dict(n, m, nv)."""
        out3 = np.zeros(3, np.int32)
        self.call("marginalize_to_prior", int(first_kf), int(max_edges), _ip(out3))
        self.dims["n_prior"] = int(out3[0])
        return dict(n=int(out3[0]), m=int(out3[1]), nv=int(out3[2]))

    def marginals(self, pairs=None, points=True, lines=True):
        """plba_compute_marginals at the current estimate: dict of numpy arrays kf (K,15,15), pairs (n,15,15), pt (Np,3,3),
        pt_status (Np,), ln (Nl,6,6), ln_status (Nl,) and n_excluded (points, lines)."""
        sz = np.zeros(6, np.int32)
        self.call("get_sizes", _ip(sz))
        K, Np, Nl = int(sz[0]), int(sz[1]), int(sz[2])
        pr = np.zeros((0, 2), np.int32) if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        kf = np.zeros((K, 15, 15)); pc = np.zeros((max(len(pr), 1), 15, 15))
        pt = np.zeros((max(Np, 1), 3, 3)); ps = np.zeros(max(Np, 1), np.uint8)
        ln = np.zeros((max(Nl, 1), 6, 6)); ls = np.zeros(max(Nl, 1), np.uint8)
        m = Marginals()
        m.want = 1 | (2 if len(pr) else 0) | (4 if points else 0) | (8 if lines else 0)
        m.n_pairs = len(pr)
        m.pairs = _ip(pr) if len(pr) else None
        m.kf_cov, m.pair_cov, m.pt_cov, m.ln_cov = _dp(kf), _dp(pc), _dp(pt), _dp(ln)
        m.pt_status, m.ln_status = _up(ps), _up(ls)
        self.call("compute_marginals", C.byref(m))
        out = dict(kf=kf, pairs=pc[:len(pr)], n_excluded=(int(m.n_excluded[0]), int(m.n_excluded[1])))
        if points:
            out["pt"], out["pt_status"] = pt[:Np], ps[:Np]
        if lines:
            out["ln"], out["ln_status"] = ln[:Nl], ls[:Nl]
        return out

    def get_prior(self):
        """plba_get_prior: the current prior, as marginalize() returns it."""
        pr = Prior()
        self.call("get_prior", C.byref(pr))
        return self._prior_dict(pr)

    def _prior_dict(self, pr):
        n, nv = pr.n, pr.nv

        def arr(p, cnt, dt):
            return np.ctypeslib.as_array(p, shape=(cnt,)).astype(dt).copy() if cnt else np.zeros(0, dt)
        size = arr(pr.size, nv, np.int32)
        nx = int(sum(10 if s == 9 else 6 for s in size))
        out = dict(n=n, m=pr.m, vid=arr(pr.vid, nv, np.int32), size=size, idx=arr(pr.idx, nv, np.int32),
                   x0=arr(pr.x0, nx, np.float64),
                   J0=arr(pr.J0, n * n, np.float64).reshape(n, n).T.copy(),  # colmajor -> J0[r, c]
                   r0=arr(pr.r0, n, np.float64),
                   Ar=arr(pr.Ar, n * n, np.float64).reshape(n, n) if pr.Ar else None, br=arr(pr.br, n, np.float64) if pr.br else None)
        self.lib.fn["prior_free"](C.byref(pr))
        return out

    def lba_visual(self, T_kf_w, kf_loc, xyz, pq, po_pt, po_kf, uv, lo_ln, lo_kf, l3, cam, **opts):
        """MapHandler::levMarquardtOptimizationLBA (src/mapHandler.cpp:1441-2098) on the arrays of include/plba.h;
        returns the optimised poses / landmarks, the moved flags and the run's statistics."""
        o = LbaOptions()
        self.lib.fn["lba_default_options"](C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError("unknown LBA option %r" % k)
            setattr(o, k, v)
        T = _f64(T_kf_w).reshape(-1, 16).copy(); K = T.shape[0]
        xyz = _f64(xyz).reshape(-1, 3).copy(); pq = _f64(pq).reshape(-1, 6).copy()
        po_pt, po_kf, lo_ln, lo_kf, loc = _i32(po_pt), _i32(po_kf), _i32(lo_ln), _i32(lo_kf), _i32(kf_loc)
        uv, l3 = _f64(uv).reshape(-1, 2), _f64(l3).reshape(-1, 3)
        Tout = np.zeros((K, 16)); pm = np.zeros(max(len(xyz), 1), np.uint8); lm = np.zeros(max(len(pq), 1), np.uint8)
        st = LbaStats()
        self.call("lba_visual", C.byref(o), K, _dp(T), _ip(loc), len(xyz), _dp(xyz), len(pq), _dp(pq),
                  len(po_pt), _ip(po_pt), _ip(po_kf), _dp(uv), len(lo_ln), _ip(lo_ln), _ip(lo_kf), _dp(l3),
                  float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), _dp(Tout), _up(pm), _up(lm), C.byref(st))
        return dict(T=Tout.reshape(K, 4, 4), xyz=xyz, pq=pq, pt_moved=pm[:len(xyz)].astype(bool), ln_moved=lm[:len(pq)].astype(bool),
                    iterations=st.iterations, updates=st.updates, err_first=st.err_first, err_last=st.err_last, lam=st.lam,
                    solver_failed=st.solver_failed)

    # -- diagnostics -------------------------------------------------------------------------
    def debug_build(self, lam, do_solve=False):
        self.call("debug_build", float(lam), int(do_solve))

    def debug_get(self, what):
        n = C.c_size_t(0)
        self.call("debug_get", what.encode(), None, 0, C.byref(n))
        a = np.zeros(max(n.value, 1))
        self.call("debug_get", what.encode(), _dp(a), n.value, C.byref(n))
        return a[:n.value]

    def dense_solve(self, A, b, entry="dense_solve"):
        A = _f64(A); b = _f64(b)
        n = len(b)
        x = np.zeros(n); ok = C.c_int(0)
        self.call(entry, n, _dp(A), _dp(b), _dp(x), C.byref(ok))
        return x, bool(ok.value)

    def debug_dense_solve(self, A, b):
        return self.dense_solve(A, b, entry="debug_dense_solve")

    def pgo(self, pose12, ei, ej, meas12, info=None, fixed=None, iters=100, user_lambda=0.0, initial_guess=False, trace_cap=None):
        """plba_optimize_pose_graph: g2o VertexSE3 / EdgeSE3 under the Levenberg loop, on the device.  pose12 (nv, 12) and meas12 (ne, 12):
        R row-major, t; info (ne, 6, 6) or None (identity); fixed (nv,) or None.  Returns (poses (nv, 12), stats dict, trace list of dicts);
        the problem's window is not touched."""
        X = _f64(pose12)
        if X.ndim != 2 or X.shape[1] != 12 or X.shape[0] < 1:
            raise ValueError("pose12 must be (nv, 12), nv >= 1")
        X = X.copy()
        nv = X.shape[0]
        ei, ej = _i32(np.asarray(ei).ravel()), _i32(np.asarray(ej).ravel())
        Z = _f64(meas12)
        ne = len(ei)
        if len(ej) != ne or Z.size != 12 * ne:
            raise ValueError("ei, ej and meas12 must describe the same %d edges" % ne)
        Z = Z.reshape(ne, 12)
        om = None if info is None else _f64(info).reshape(-1)
        if om is not None and om.size != 36 * ne:
            raise ValueError("info must be (ne, 6, 6)")
        fx = None if fixed is None else _u8(np.asarray(fixed).astype(bool))
        if fx is not None and fx.size != nv:
            raise ValueError("fixed must have nv entries")
        g = PoseGraph(nv, _dp(X), _up(fx), ne, _ip(ei), _ip(ej), _dp(Z), _dp(om))
        cap = max(1, int(iters) * 10) if trace_cap is None else int(trace_cap)
        rows = (TraceRow * max(cap, 1))()
        st = Stats()
        ntr = C.c_int(0)
        self.call("optimize_pose_graph", C.byref(g), int(iters), float(user_lambda), 1 if initial_guess else 0, C.byref(st), rows, cap, C.byref(ntr))
        stats = dict(iterations=st.iterations, trials=st.trials, stop_reason=st.stop_reason, solver_failures=st.solver_failures,
                     chi2_initial=st.chi2_initial, chi2_final=st.chi2_final, lambda_final=st.lambda_final, ms_total=st.ms_total, n_trace=ntr.value)
        trace = [dict(iteration=r.iteration, trial=r.trial, accepted=r.accepted, solver_ok=r.solver_ok, lam=r.lam, chi2_current=r.chi2_current,
                      chi2_trial=r.chi2_trial, scale=r.scale, rho=r.rho) for r in rows[:min(ntr.value, cap)]]
        return X, stats, trace

    def pgo_marginals(self, pose12, ei, ej, meas12, info=None, fixed=None, pairs=None):
        """plba_pose_graph_marginals: the 6 x 6 marginal covariance of every vertex of the pose graph at pose12 and Cov(x_i, x_j) of the
        pairs (n, 2) given, from the sparse factor.  Arguments as pgo().  Returns dict(v_cov (nv, 6, 6), v_status (nv,), pair_cov (n, 6, 6),
        pair_status (n,), n_status (4,)); the problem's window is not touched."""
        X = _f64(pose12)
        if X.ndim != 2 or X.shape[1] != 12 or X.shape[0] < 1:
            raise ValueError("pose12 must be (nv, 12), nv >= 1")
        nv = X.shape[0]
        ei, ej = _i32(np.asarray(ei).ravel()), _i32(np.asarray(ej).ravel())
        Z = _f64(meas12)
        ne = len(ei)
        if len(ej) != ne or Z.size != 12 * ne:
            raise ValueError("ei, ej and meas12 must describe the same %d edges" % ne)
        Z = Z.reshape(ne, 12)
        om = None if info is None else _f64(info).reshape(-1)
        if om is not None and om.size != 36 * ne:
            raise ValueError("info must be (ne, 6, 6)")
        fx = None if fixed is None else _u8(np.asarray(fixed).astype(bool))
        if fx is not None and fx.size != nv:
            raise ValueError("fixed must have nv entries")
        g = PoseGraph(nv, _dp(X), _up(fx), ne, _ip(ei), _ip(ej), _dp(Z), _dp(om))
        pr = np.zeros((0, 2), np.int32) if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        vc = np.zeros((nv, 6, 6)); vs = np.zeros(nv, np.uint8)
        pc = np.zeros((max(len(pr), 1), 6, 6)); ps = np.zeros(max(len(pr), 1), np.uint8)
        m = PgoMarginals()
        m.want = 1 | (2 if len(pr) else 0)
        m.n_pairs = len(pr)
        m.pairs = _ip(pr) if len(pr) else None
        m.v_cov, m.v_status, m.pair_cov, m.pair_status = _dp(vc), _up(vs), _dp(pc), _up(ps)
        self.call("pose_graph_marginals", C.byref(g), C.byref(m))
        return dict(v_cov=vc, v_status=vs, pair_cov=pc[:len(pr)], pair_status=ps[:len(pr)], n_status=np.array(list(m.n_status), np.int32))

    def refine_landmarks(self, select_point=None, select_line=None, **opts):
        """plba_refine_landmarks: every selected landmark fitted to the keyframes the device holds (structure-only LM, one launch).
        select_point / select_line: boolean masks or None (all); opts: max_iters, max_trials, lambda_init.  Returns a dict of the
        call's plba_refine_stats plus status / iters / trials, one entry per landmark (points, then lines)."""
        o = RefineOptions()
        self.lib.fn["refine_default_options"](C.byref(o))
        for k, v in opts.items():
            if k not in ("max_iters", "max_trials", "lambda_init"):
                raise TypeError("unknown refine option %r" % k)
            setattr(o, k, v)
        sz = np.zeros(6, np.int32)
        self.call("get_sizes", _ip(sz))
        Np, Nl = int(sz[1]), int(sz[2])
        sp = None if select_point is None else _u8(np.asarray(select_point).astype(bool))
        sl = None if select_line is None else _u8(np.asarray(select_line).astype(bool))
        if (sp is not None and sp.size != Np) or (sl is not None and sl.size != Nl):
            raise ValueError("select masks must have one entry per point / line")
        status, iters, trials = np.zeros(max(Np + Nl, 1), np.uint8), np.zeros(max(Np + Nl, 1), np.int32), np.zeros(max(Np + Nl, 1), np.int32)
        o.select_point, o.select_line = _up(sp), _up(sl)
        o.status, o.iters, o.trials = _up(status), _ip(iters), _ip(trials)
        st = RefineStats()
        self.call("refine_landmarks", C.byref(o), C.byref(st))
        return dict(n_refined=st.n_refined, n_skipped=st.n_skipped, n_exhausted=st.n_exhausted, iterations=st.iterations, trials=st.trials,
                    chi2_before=st.chi2_before, chi2_after=st.chi2_after, ms_total=st.ms_total,
                    status=status[:Np + Nl], iters=iters[:Np + Nl], trials_per_landmark=trials[:Np + Nl])

    def relative_pose(self, P3, uv, sPeP, l3, cam, T0=None, pt_inlier=None, ln_inlier=None, **opts):
        """plba_relative_pose: B loop-closure candidates verified in one launch.  P3 / uv / sPeP / l3: lists of B arrays ((n, 3), (n, 2),
        (m, 6), (m, 3); an empty array or None for a candidate without points or lines); cam = (fx, fy, cx, cy); T0: (B, 4, 4) or None
        (identity); pt_inlier / ln_inlier: lists of B masks or None (all); opts: the fields of plba_relpose_options.  Returns a dict of
        arrays over the candidates — T_inc (B, 4, 4), pose_inc (B, 6), H (B, 6, 6), e, cov_eig (B, 6), t, r, n_inliers, iters (B, 2), status,
        accepted, lc_res .. lc_rot — and pt_inlier / ln_inlier, lists of B boolean masks as the cut left them."""
        o = RelposeOptions()
        self.lib.fn["relpose_default_options"](C.byref(o))
        for k, v in opts.items():
            if k == "reserved" or not hasattr(o, k):
                raise TypeError("unknown relative-pose option %r" % k)
            setattr(o, k, v)
        B = len(P3)
        if not (len(uv) == len(sPeP) == len(l3) == B):
            raise ValueError("P3, uv, sPeP and l3 must list the same candidates")

        def csr(lists, width):
            arrs = [np.zeros((0, width)) if a is None else _f64(a).reshape(-1, width) for a in lists]
            start = np.zeros(len(arrs) + 1, np.int32)
            start[1:] = np.cumsum([len(a) for a in arrs])
            return start, (np.concatenate(arrs) if arrs else np.zeros((0, width)))
        ps, P = csr(P3, 3); ps2, U2 = csr(uv, 2); ls, PQ = csr(sPeP, 6); ls2, L3 = csr(l3, 3)
        if not (np.array_equal(ps, ps2) and np.array_equal(ls, ls2)):
            raise ValueError("a candidate's P3 / uv or sPeP / l3 differ in length")

        def masks(m, start):
            if m is None:
                return np.ones(max(int(start[-1]), 1), np.uint8)
            if len(m) != B or any(len(np.asarray(a).ravel()) != start[b + 1] - start[b] for b, a in enumerate(m)):
                raise ValueError("a mask list must have one entry per candidate and one flag per feature")
            flat = np.concatenate([np.asarray(a).ravel().astype(bool) for a in m]) if B else np.zeros(0, bool)
            return np.concatenate([flat.astype(np.uint8), np.zeros(1 if flat.size == 0 else 0, np.uint8)])
        pm, lm = masks(pt_inlier, ps), masks(ln_inlier, ls)
        T = None if T0 is None else _f64(T0).reshape(-1, 16).copy()
        if T is not None and T.shape[0] != B:
            raise ValueError("T0 must be (B, 4, 4)")
        res = (RelposeResult * max(B, 1))()
        self.call("relative_pose", C.byref(o), B, _ip(ps), _dp(P) if len(P) else None, _dp(U2) if len(U2) else None, _ip(ls),
                  _dp(PQ) if len(PQ) else None, _dp(L3) if len(L3) else None, float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]),
                  _dp(T), _up(pm), _up(lm), res)
        out = dict(T_inc=np.array([list(r.T_inc16) for r in res[:B]]).reshape(B, 4, 4), pose_inc=np.array([list(r.pose_inc6) for r in res[:B]]).reshape(B, 6),
                   H=np.array([list(r.H36) for r in res[:B]]).reshape(B, 6, 6), cov_eig=np.array([list(r.cov_eig6) for r in res[:B]]).reshape(B, 6),
                   iters=np.array([list(r.iters) for r in res[:B]], np.int32).reshape(B, 2))
        for k in ("e", "t", "r"):
            out[k] = np.array([getattr(r, k) for r in res[:B]], np.float64)
        for k in ("n_inliers", "status", "accepted", "lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot"):
            out[k] = np.array([getattr(r, k) for r in res[:B]], np.int32)
        out["pt_inlier"] = [pm[ps[b]:ps[b + 1]].astype(bool) for b in range(B)]
        out["ln_inlier"] = [lm[ls[b]:ls[b + 1]].astype(bool) for b in range(B)]
        return out

    def track_pose(self, P3, uv, pt_sigma2, sPeP, l3, spl_epl, ln_sigma2, cam, T0=None, pt_inlier=None, ln_inlier=None, **opts):
        """plba_track_pose: B frame-to-frame pose estimates (StereoFrameHandler::optimizePose) in one launch.  P3 / uv / pt_sigma2 / sPeP / l3 /
        spl_epl / ln_sigma2: lists of B arrays ((n, 3), (n, 2), (n,), (m, 6), (m, 3), (m, 4), (m,); an empty array or None for a problem without
        points or lines); cam = (fx, fy, cx, cy); T0: (B, 4, 4) start poses or None (identity); pt_inlier / ln_inlier: lists of B masks or None
        (all); opts: the fields of plba_track_options.  Returns a dict of arrays over the problems — DT, T_opt (B, 4, 4), H, cov (B, 6, 6),
        cov_eig (B, 6), err, pt_mean, pt_stdv, ln_mean, ln_stdv, n_inliers_pt, n_inliers_ln, iters (B, 3), path, status, good — and
        pt_inlier / ln_inlier, lists of B boolean masks as the cut left them."""
        o = TrackOptions()
        self.lib.fn["track_default_options"](C.byref(o))
        for k, v in opts.items():
            if k == "reserved" or not hasattr(o, k):
                raise TypeError("unknown track-pose option %r" % k)
            setattr(o, k, v)
        B = len(P3)
        if not (len(uv) == len(pt_sigma2) == len(sPeP) == len(l3) == len(spl_epl) == len(ln_sigma2) == B):
            raise ValueError("the feature lists must list the same problems")

        def csr(lists, width):
            arrs = [np.zeros((0, width)) if a is None else _f64(a).reshape(-1, width) for a in lists]
            start = np.zeros(len(arrs) + 1, np.int32)
            start[1:] = np.cumsum([len(a) for a in arrs])
            return start, (np.concatenate(arrs) if arrs else np.zeros((0, width)))
        ps, P = csr(P3, 3); ps2, U2 = csr(uv, 2); ps3, S2P = csr(pt_sigma2, 1)
        ls, PQ = csr(sPeP, 6); ls2, L3 = csr(l3, 3); ls3, SE = csr(spl_epl, 4); ls4, S2L = csr(ln_sigma2, 1)
        if not (np.array_equal(ps, ps2) and np.array_equal(ps, ps3) and np.array_equal(ls, ls2) and np.array_equal(ls, ls3) and np.array_equal(ls, ls4)):
            raise ValueError("a problem's point arrays or line arrays differ in length")

        def masks(m, start):
            if m is None:
                return np.ones(max(int(start[-1]), 1), np.uint8)
            if len(m) != B or any(len(np.asarray(a).ravel()) != start[b + 1] - start[b] for b, a in enumerate(m)):
                raise ValueError("a mask list must have one entry per problem and one flag per feature")
            flat = np.concatenate([np.asarray(a).ravel().astype(bool) for a in m]) if B else np.zeros(0, bool)
            return np.concatenate([flat.astype(np.uint8), np.zeros(1 if flat.size == 0 else 0, np.uint8)])
        pm, lm = masks(pt_inlier, ps), masks(ln_inlier, ls)
        T = None if T0 is None else _f64(T0).reshape(-1, 16).copy()
        if T is not None and T.shape[0] != B:
            raise ValueError("T0 must be (B, 4, 4)")
        res = (TrackResult * max(B, 1))()
        opt_p = lambda a: _dp(a) if len(a) else None
        self.call("track_pose", C.byref(o), B, _ip(ps), opt_p(P), opt_p(U2), opt_p(S2P), _ip(ls), opt_p(PQ), opt_p(L3), opt_p(SE), opt_p(S2L),
                  float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), _dp(T), _up(pm), _up(lm), res)
        arr = lambda f, shape: np.array([list(getattr(r, f)) for r in res[:B]], np.float64).reshape((B,) + shape)
        out = dict(DT=arr("DT16", (4, 4)), T_opt=arr("T_opt16", (4, 4)), H=arr("H36", (6, 6)), cov=arr("cov36", (6, 6)), cov_eig=arr("cov_eig6", (6,)),
                   iters=np.array([list(r.iters) for r in res[:B]], np.int32).reshape(B, 3))
        for k in ("err", "pt_mean", "pt_stdv", "ln_mean", "ln_stdv"):
            out[k] = np.array([getattr(r, k) for r in res[:B]], np.float64)
        for k in ("n_inliers_pt", "n_inliers_ln", "path", "status", "good"):
            out[k] = np.array([getattr(r, k) for r in res[:B]], np.int32)
        out["pt_inlier"] = [pm[ps[b]:ps[b + 1]].astype(bool) for b in range(B)]
        out["ln_inlier"] = [lm[ls[b]:ls[b + 1]].astype(bool) for b in range(B)]
        return out

    def track_inertial(self, anchor_free, state_i, state_j, preint, info_pvr, info_bias, prior_state, prior_info, gw, Pw, uv, pt_inv_sigma2, sPeP, l3,
                       ln_inv_sigma2, cam, Rbc, Pbc, pt_inlier=None, ln_inlier=None, **opts):
        """plba_track_inertial: B motion-only visual-inertial optimisations of two consecutive states in one launch.  anchor_free: B flags or
        None (every anchor fixed); state_i / state_j (B, 22), preint (B, 142), info_pvr (B, 9, 9), info_bias (B, 6, 6); prior_state (B, 22) and
        prior_info (B, 15, 15) or None when no anchor is free; gw (3,); Pw / uv / pt_inv_sigma2 / sPeP / l3 / ln_inv_sigma2: lists of B arrays
        ((n, 3), (n, 2), (n,), (m, 6), (m, 3), (m,); an empty array or None for a problem without points or lines); cam = (fx, fy, cx, cy), Rbc
        (3, 3), Pbc (3,); pt_inlier / ln_inlier: lists of B masks or None (all); opts: the fields of plba_vitrack_options.  Returns a dict of
        arrays over the problems — state_i, state_j (B, 22), H (B, 30, 30), next_prior (B, 15, 15), chi2_initial, chi2_final, lambda_final,
        iterations, stop_reason (B, 8), trials, solver_failures, n_inliers_pt, n_inliers_ln, status — and pt_inlier / ln_inlier, lists of B
        boolean masks as the last gate left them."""
        o = VitrackOptions()
        self.lib.fn["vitrack_default_options"](C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError("unknown track-inertial option %r" % k)
            setattr(o, k, v)
        B = len(Pw)
        if not (len(uv) == len(pt_inv_sigma2) == len(sPeP) == len(l3) == len(ln_inv_sigma2) == B):
            raise ValueError("the feature lists must list the same problems")

        def csr(lists, width):
            arrs = [np.zeros((0, width)) if a is None else _f64(a).reshape(-1, width) for a in lists]
            start = np.zeros(len(arrs) + 1, np.int32)
            start[1:] = np.cumsum([len(a) for a in arrs])
            return start, (np.concatenate(arrs) if arrs else np.zeros((0, width)))
        ps, P = csr(Pw, 3); ps2, U2 = csr(uv, 2); ps3, WP = csr(pt_inv_sigma2, 1)
        ls, PQ = csr(sPeP, 6); ls2, L3 = csr(l3, 3); ls3, WL = csr(ln_inv_sigma2, 1)
        if not (np.array_equal(ps, ps2) and np.array_equal(ps, ps3) and np.array_equal(ls, ls2) and np.array_equal(ls, ls3)):
            raise ValueError("a problem's point arrays or line arrays differ in length")

        def masks(m, start):
            if m is None:
                return np.ones(max(int(start[-1]), 1), np.uint8)
            if len(m) != B or any(len(np.asarray(a).ravel()) != start[b + 1] - start[b] for b, a in enumerate(m)):
                raise ValueError("a mask list must have one entry per problem and one flag per feature")
            flat = np.concatenate([np.asarray(a).ravel().astype(bool) for a in m]) if B else np.zeros(0, bool)
            return np.concatenate([flat.astype(np.uint8), np.zeros(1 if flat.size == 0 else 0, np.uint8)])
        pm, lm = masks(pt_inlier, ps), masks(ln_inlier, ls)

        def rows(a, n, what):
            if a is None:
                return None
            a = _f64(a).reshape(-1, n).copy()
            if a.shape[0] != B:
                raise ValueError("%s must have one row per problem" % what)
            return a
        af = None if anchor_free is None else _u8(np.asarray(anchor_free).astype(bool))
        if af is not None and af.size != B:
            raise ValueError("anchor_free must have one flag per problem")
        si, sj, pre, ip, ib = rows(state_i, 22, "state_i"), rows(state_j, 22, "state_j"), rows(preint, 142, "preint"), rows(info_pvr, 81, "info_pvr"), rows(info_bias, 36, "info_bias")
        pst, pin = rows(prior_state, 22, "prior_state"), rows(prior_info, 225, "prior_info")
        g, R, t = _f64(gw, (3,)), _f64(Rbc, (9,)), _f64(Pbc, (3,))
        res = (VitrackResult * max(B, 1))()
        opt_p = lambda a: _dp(a) if len(a) else None
        self.call("track_inertial", C.byref(o), B, _up(af), _dp(si), _dp(sj), _dp(pre), _dp(ip), _dp(ib), _dp(pst), _dp(pin), _dp(g), _ip(ps), opt_p(P), opt_p(U2),
                  opt_p(WP), _ip(ls), opt_p(PQ), opt_p(L3), opt_p(WL), float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), _dp(R), _dp(t), _up(pm), _up(lm), res)
        rec = np.frombuffer(res, dtype=VITRACK_RESULT_DT, count=B)      # (one view of the B structs: H alone is 900 numbers a problem)
        out = {k: rec[f].copy() for k, f in (("state_i", "state_i22"), ("state_j", "state_j22"), ("H", "H900"), ("next_prior", "next_prior_info225"))}
        for k in ("chi2_initial", "chi2_final", "lambda_final", "iterations", "stop_reason", "trials", "solver_failures", "n_inliers_pt", "n_inliers_ln", "status"):
            out[k] = rec[k].copy()
        out["pt_inlier"] = [pm[ps[b]:ps[b + 1]].astype(bool) for b in range(B)]
        out["ln_inlier"] = [lm[ls[b]:ls[b + 1]].astype(bool) for b in range(B)]
        return out

    def match_descriptors(self, desc1, desc2, nnr_b=None, want_nn3=False, **opts):
        """plba_match_descriptors: StVO::match for B problems in one launch.  desc1 / desc2: lists of B uint8 arrays (n, 32) (an empty array
        or None for an empty side); nnr_b: B ratios or None (opts' nnr for all); opts: the fields of plba_match_options.  Returns a dict:
        matches_12, a list of B int32 arrays (index into the problem's desc2, or -1), n_matches (B,), and with want_nn3 nn3, a list of B
        (n, 3) arrays (best index, d0, d1 of the search 1 -> 2)."""
        o = MatchOptions()
        self.lib.fn["match_default_options"](C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError("unknown match option %r" % k)
            setattr(o, k, v)
        B = len(desc1)
        if len(desc2) != B:
            raise ValueError("desc1 and desc2 must list the same problems")
        sa, A = _desc_csr(desc1); sb, D2 = _desc_csr(desc2)
        nb = None if nnr_b is None else np.ascontiguousarray(nnr_b, dtype=np.float32)
        if nb is not None and nb.size != B:
            raise ValueError("nnr_b must have one ratio per problem")
        NA = int(sa[-1])
        m = np.full(max(NA, 1), -2, np.int32); cnt = np.full(max(B, 1), -2, np.int32)
        nn3 = np.full((max(NA, 1), 3), -2, np.int32) if want_nn3 else None
        self.call("match_descriptors", C.byref(o), B, _ip(sa), _up(A) if len(A) else None, _ip(sb), _up(D2) if len(D2) else None,
                  None if nb is None else nb.ctypes.data_as(C.POINTER(C.c_float)), _ip(m), _ip(cnt), _ip(nn3))
        out = dict(matches_12=[m[sa[b]:sa[b + 1]].copy() for b in range(B)], n_matches=cnt[:B].copy())
        if want_nn3:
            out["nn3"] = [nn3[sa[b]:sa[b + 1]].copy() for b in range(B)]
        return out

    def verify_loop_candidates(self, kf0, kf1, cam, want_masks=True, **opts):
        """plba_verify_loop_candidates: isLoopClosure for B candidates with one wait.  kf0 / kf1: lists of B dicts — kf0[b]: pdesc (n, 32),
        P3 (n, 3), ldesc (m, 32), sPeP (m, 6); kf1[b]: pdesc, uv (n, 2), ldesc, l3 (m, 3); cam = (fx, fy, cx, cy); opts: use_points,
        use_lines, lc_inlier_ratio, nnr_pt, nnr_ln, best_lr (both kinds) and the fields of plba_relpose_options.  Returns a dict: pt_match /
        ln_match (lists of B int32 arrays), pt_inlier / ln_inlier (lists of B boolean masks), common_pt, common_ls, ratio_ok, inl_ratio_pt,
        inl_ratio_ls (arrays over B) and relpose, the dict Problem.relative_pose returns without its masks."""
        o = LoopOptions()
        self.lib.fn["loop_default_options"](C.byref(o))
        for k, v in opts.items():
            if k == "nnr_pt":
                o.match_pt.nnr = v
            elif k == "nnr_ln":
                o.match_ln.nnr = v
            elif k == "best_lr":
                o.match_pt.best_lr = o.match_ln.best_lr = int(v)
            elif k in ("use_points", "use_lines", "lc_inlier_ratio"):
                setattr(o, k, v)
            elif k != "reserved" and hasattr(o.relpose, k):
                setattr(o.relpose, k, v)
            else:
                raise TypeError("unknown loop option %r" % k)
        B = len(kf0)
        if len(kf1) != B:
            raise ValueError("kf0 and kf1 must list the same candidates")

        def csr(dicts, key, width):
            arrs = [np.zeros((0, width)) if d.get(key) is None else _f64(d[key]).reshape(-1, width) for d in dicts]
            start = np.zeros(len(arrs) + 1, np.int32)
            start[1:] = np.cumsum([len(a) for a in arrs])
            return start, (np.concatenate(arrs) if arrs else np.zeros((0, width)))
        pa, DPA = _desc_csr([d.get("pdesc") for d in kf0]); pa2, P3 = csr(kf0, "P3", 3)
        pb, DPB = _desc_csr([d.get("pdesc") for d in kf1]); pb2, UV = csr(kf1, "uv", 2)
        la, DLA = _desc_csr([d.get("ldesc") for d in kf0]); la2, PQ = csr(kf0, "sPeP", 6)
        lb, DLB = _desc_csr([d.get("ldesc") for d in kf1]); lb2, L3 = csr(kf1, "l3", 3)
        if not (np.array_equal(pa, pa2) and np.array_equal(pb, pb2) and np.array_equal(la, la2) and np.array_equal(lb, lb2)):
            raise ValueError("a keyframe's descriptors and features differ in length")
        NpA, NlA = int(pa[-1]), int(la[-1])
        pm_, lm_ = np.full(max(NpA, 1), -2, np.int32), np.full(max(NlA, 1), -2, np.int32)
        pi, li = (np.zeros(max(NpA, 1), np.uint8), np.zeros(max(NlA, 1), np.uint8)) if want_masks else (None, None)
        res = (LoopResult * max(B, 1))()
        u8 = lambda a: _up(a) if len(a) else None
        dd = lambda a: _dp(a) if len(a) else None
        self.call("verify_loop_candidates", C.byref(o), B, _ip(pa), u8(DPA), dd(P3), _ip(pb), u8(DPB), dd(UV), _ip(la), u8(DLA), dd(PQ), _ip(lb), u8(DLB), dd(L3),
                  float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), _ip(pm_), _ip(lm_), _up(pi), _up(li), res)
        out = dict(pt_match=[pm_[pa[b]:pa[b + 1]].copy() for b in range(B)], ln_match=[lm_[la[b]:la[b + 1]].copy() for b in range(B)])
        if want_masks:
            out["pt_inlier"] = [pi[pa[b]:pa[b + 1]].astype(bool) for b in range(B)]
            out["ln_inlier"] = [li[la[b]:la[b + 1]].astype(bool) for b in range(B)]
        for k in ("common_pt", "common_ls", "ratio_ok"):
            out[k] = np.array([getattr(r, k) for r in res[:B]], np.int32)
        for k in ("inl_ratio_pt", "inl_ratio_ls"):
            out[k] = np.array([getattr(r, k) for r in res[:B]], np.float64)
        out["relpose"] = _relpose_dict([r.relpose for r in res[:B]])
        return out

    def bow_set_vocabulary(self, kind, voc, weighting=0, scoring=0):
        """plba_bow_set_vocabulary: voc is a dict with parent (n,), desc (n, 32) uint8, weight (n,), word_id (n,) and optionally k, L; kind 0 =
        points, 1 = lines.  Drops the database."""
        parent, desc, weight, word = _i32(voc["parent"]), _u8(voc["desc"]).reshape(-1, 32), _f64(voc["weight"]), _i32(voc["word_id"])
        n = len(parent)
        if not (len(desc) == len(weight) == len(word) == n):
            raise ValueError("the vocabulary's arrays differ in length")
        self.call("bow_set_vocabulary", int(kind), int(voc.get("k", 0)), int(voc.get("L", 0)), int(weighting), int(scoring), n, _ip(parent), _up(desc), _dp(weight),
                  _ip(word))

    def bow_transform(self, kind, desc):
        """plba_bow_transform: desc is a list of B (n, 32) uint8 arrays.  Returns a dict of lists over B: word (int32, -1: stopped), bow_id,
        bow_val (the normalised vector, ids ascending)."""
        st, D = _desc_csr(desc)
        B, N = len(desc), int(st[-1])
        word, ids, vals, nnz = np.full(max(N, 1), -2, np.int32), np.full(max(N, 1), -2, np.int32), np.zeros(max(N, 1)), np.full(max(B, 1), -2, np.int32)
        self.call("bow_transform", int(kind), B, _ip(st), _up(D) if N else None, _ip(word), _ip(ids), _dp(vals), _ip(nnz))
        return dict(word=[word[st[b]:st[b + 1]].copy() for b in range(B)], bow_id=[ids[st[b]:st[b] + nnz[b]].copy() for b in range(B)],
                    bow_val=[vals[st[b]:st[b] + nnz[b]].copy() for b in range(B)])

    def bow_insert_keyframes(self, kfs, cov=None, want_bow=False, want_scores=True, **opts):
        """plba_bow_insert_keyframes: kfs is a list of B dicts — pdesc (n, 32), pl (n, 2), ldesc (m, 32), spl_epl (m, 4) (a missing key is an
        empty kind); cov: None or a list of B int arrays, cov[b] the covisibility column of keyframe b (first_index + b entries); opts: the
        fields of plba_bow_options.  Returns a dict: first_index, and lists over B of score_p, score_l, score (float64) and score_f32, each
        idx + 1 long (not with want_scores=False: the columns are then not read back); with cov, the fields of plba_bow_candidate as arrays over B (topk: (B, 16)); with want_bow, pt / ln dicts as
        bow_transform returns them."""
        o = BowOptions()
        self.lib.fn["bow_default_options"](C.byref(o))
        for k, v in opts.items():
            if k == "reserved" or not hasattr(o, k):
                raise TypeError("unknown bow option %r" % k)
            setattr(o, k, int(v))
        B = len(kfs)
        n0 = int(self.debug_get("bow_db")[0])

        def csr(key, width):
            arrs = [np.zeros((0, width)) if d.get(key) is None else _f64(d[key]).reshape(-1, width) for d in kfs]
            start = np.zeros(len(arrs) + 1, np.int32)
            start[1:] = np.cumsum([len(a) for a in arrs])
            return start, (np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros((0, width)))
        ps, DP = _desc_csr([d.get("pdesc") for d in kfs]); ps2, PL = csr("pl", 2)
        ls, DL = _desc_csr([d.get("ldesc") for d in kfs]); ls2, SE = csr("spl_epl", 4)
        if o.mode == BOW_COMBINED and not (np.array_equal(ps, ps2) and np.array_equal(ls, ls2)):
            raise ValueError("a keyframe's descriptors and positions differ in length")
        R = B * (n0 + 1) + B * (B - 1) // 2
        Ra = max(R, 1) if want_scores else 1
        sp, sl, sc, sf = np.zeros(Ra), np.zeros(Ra), np.zeros(Ra), np.zeros(Ra, np.float32)
        r = BowResult()
        r.score_cap = max(R, 1)
        if want_scores:
            r.score_p, r.score_l, r.score, r.score_f32 = _dp(sp), _dp(sl), _dp(sc), sf.ctypes.data_as(C.POINTER(C.c_float))
        Np, Nl = int(ps[-1]), int(ls[-1])
        keep = []
        if want_bow:
            for pre, N in (("pt", Np), ("ln", Nl)):
                w, i, v, z = np.full(max(N, 1), -2, np.int32), np.full(max(N, 1), -2, np.int32), np.zeros(max(N, 1)), np.zeros(max(B, 1), np.int32)
                keep.append((w, i, v, z))
                setattr(r, pre + "_word", _ip(w)); setattr(r, pre + "_bow_id", _ip(i)); setattr(r, pre + "_bow_val", _dp(v)); setattr(r, pre + "_nnz", _ip(z))
        cs = cv = cand = None
        if cov is not None:
            if len(cov) != B:
                raise ValueError("cov must list one column per keyframe")
            cols = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in cov]
            cs = np.zeros(B + 1, np.int32); cs[1:] = np.cumsum([len(c) for c in cols])
            cv = np.ascontiguousarray(np.concatenate(cols + [np.zeros(1, np.int32)]))
            cand = (BowCandidate * max(B, 1))()
            r.cand = cand
        up = lambda a: _up(a) if len(a) else None
        dd = lambda a: _dp(a) if len(a) else None
        self.call("bow_insert_keyframes", C.byref(o), B, _ip(ps), up(DP), dd(PL), _ip(ls), up(DL), dd(SE), _ip(cs), _ip(cv), C.byref(r))
        row = lambda b: b * (n0 + 1) + b * (b - 1) // 2
        out = dict(first_index=int(r.first_index))
        for k, a in (("score_p", sp), ("score_l", sl), ("score", sc), ("score_f32", sf)) if want_scores else ():
            out[k] = [a[row(b):row(b) + n0 + b + 1].copy() for b in range(B)]
        if cand is not None:
            for k in ("is_candidate", "kf_prev", "n_closest", "n_eligible"):
                out[k] = np.array([getattr(c, k) for c in cand[:B]], np.int32)
            for k in ("best_score", "lc_min_score"):
                out[k] = np.array([getattr(c, k) for c in cand[:B]], np.float64)
            out["topk"] = np.array([list(c.topk) for c in cand[:B]], np.int32).reshape(B, 16)
            out["topk_score"] = np.array([list(c.topk_score) for c in cand[:B]], np.float64).reshape(B, 16)
        if want_bow:
            for (pre, st_), (w, i, v, z) in zip((("pt", ps), ("ln", ls)), keep):
                out[pre] = dict(word=[w[st_[b]:st_[b + 1]].copy() for b in range(B)], bow_id=[i[st_[b]:st_[b] + z[b]].copy() for b in range(B)],
                                bow_val=[v[st_[b]:st_[b] + z[b]].copy() for b in range(B)])
        return out

    def bow_remove_keyframe(self, kf):
        self.call("bow_remove_keyframe", int(kf))

    def bow_reset(self):
        self.call("bow_reset")

    # -- covisibility graph -----------------------------------------------------------------------
    def _covis_options(self, opts):
        o = CovisOptions()
        self.lib.fn["covis_default_options"](C.byref(o))
        for k, v in opts.items():
            if k not in ("min_lm_ess_graph", "min_lm_cov_graph", "min_kf_local_map"):
                raise TypeError("unknown covis option %r" % k)
            setattr(o, k, int(v))
        return o

    def covis_set_map(self, K, pt_start, pt_kf, ln_start=None, ln_kf=None, live=None):
        """plba_covis_set_map: the landmarks' observation lists as CSR per kind (start: n + 1 entries, kf: the keyframe indices); a missing
        kind is empty.  Returns the info array [K, live keyframes, landmarks, point observations, line observations, device bytes]."""
        ps, pk, ls, lk = _i32(pt_start), _i32(pt_kf), _i32(ln_start), _i32(ln_kf)
        lv = _u8(live)
        if lv is not None and len(lv) != int(K):
            raise ValueError("live must have K entries")
        dims = (int(K), 0 if ps is None else len(ps) - 1, 0 if ls is None else len(ls) - 1)
        info = np.zeros(6, np.float64)
        self.call("covis_set_map", int(K), _up(lv), dims[1], _ip(ps), _ip(pk), dims[2], _ip(ls), _ip(lk), _dp(info))
        self._covis_dims = dims      # (a refused call leaves the resident map, and these, as they were)
        return info

    def covis_reset(self):
        self.call("covis_reset")
        self._covis_dims = None

    def covis_rows(self, kf, min_count=0, cap=None):
        """plba_covis_rows: (row_start, col, cnt) of the listed keyframes' sparse rows.  cap=None: the capacity is taken from a first,
        refused call's answer when a guess of 64 entries a row does not hold (a second device call); a given cap too small raises."""
        kf = _i32(np.atleast_1d(kf))
        n = len(kf)
        rs = np.zeros(n + 1, np.int32)
        guess = 64 * n + 64 if cap is None else int(cap)
        for attempt in range(2):
            col, cnt = np.zeros(max(guess, 1), np.int32), np.zeros(max(guess, 1), np.int32)
            rc = self.lib.fn["covis_rows"](self._h, n, _ip(kf), int(min_count), _ip(rs), guess, _ip(col), _ip(cnt))
            if rc == -1 and cap is None and attempt == 0 and guess < rs[n] < 2 ** 31 - 1:
                guess = int(rs[n])
                continue
            self._ck(rc)
            return rs, col[:rs[n]].copy(), cnt[:rs[n]].copy()

    def covis_column(self, idx):
        """plba_covis_column: full_graph[i][idx] for i < idx, the cov array of plba_bow_insert_keyframes"""
        cov = np.zeros(max(int(idx), 1), np.int32)
        self.call("covis_column", int(idx), _ip(cov))
        return cov[:max(int(idx), 0)]

    def covis_pose_graph(self, pose12, loop_ij=None, loop_meas12=None, edge_cap=None, **opts):
        """plba_covis_pose_graph over the first len(pose12) keyframes: (ei, ej, meas12), the covisibility edges in the order of the
        reference's double loop, then the loop edges; the arrays drop into Problem.pgo.  edge_cap=None: as covis_rows' cap."""
        o = self._covis_options(opts)
        pose = _f64(pose12, (-1, 12))
        nv = len(pose)
        lij = None if loop_ij is None else _i32(loop_ij).reshape(-1, 2)
        lm = None if loop_meas12 is None else _f64(loop_meas12, (-1, 12))
        nl = 0 if lij is None else len(lij)
        if nl and (lm is None or len(lm) != nl):
            raise ValueError("loop_meas12 must have one row per loop edge")
        guess = 8 * nv + nl + 64 if edge_cap is None else int(edge_cap)
        ne = C.c_int(0)
        for attempt in range(2):
            ei, ej, z = np.zeros(max(guess, 1), np.int32), np.zeros(max(guess, 1), np.int32), np.zeros((max(guess, 1), 12), np.float64)
            rc = self.lib.fn["covis_pose_graph"](self._h, C.byref(o), nv, _dp(pose), nl, _ip(lij), _dp(lm), guess, _ip(ei), _ip(ej), _dp(z), C.byref(ne))
            if rc == -1 and edge_cap is None and attempt == 0 and guess < ne.value < 2 ** 31 - 1:
                guess = ne.value
                continue
            self._ck(rc)
            return ei[:ne.value].copy(), ej[:ne.value].copy(), z[:ne.value].copy()

    def covis_local_map(self, kf, **opts):
        """plba_covis_local_map: dict of kf_local (K), pt_local (Np), ln_local (Nl) as uint8 flags and counts (3)"""
        o = self._covis_options(opts)
        K, Np, Nl = self._covis_dims if getattr(self, "_covis_dims", None) else (int(self.debug_get("covis_map")[0]), 0, 0)
        fk, fp, fl = np.zeros(max(K, 1), np.uint8), np.zeros(max(Np, 1), np.uint8), np.zeros(max(Nl, 1), np.uint8)
        c3 = np.zeros(3, np.int32)
        self.call("covis_local_map", C.byref(o), int(kf), _up(fk), _up(fp), _up(fl), _ip(c3))
        return dict(kf_local=fk[:K], pt_local=fp[:Np], ln_local=fl[:Nl], counts=c3)

    def preintegrate(self, sample_start, t, gyr, acc, t_prev, t_curr, bg, ba, gyr_meas_cov, acc_meas_cov):
        """KeyFrame::ComputeIMUPreIntSinceLastFrame for M intervals (plba_preintegrate); time stamps as np.longdouble."""
        ss = np.ascontiguousarray(sample_start, dtype=np.int32)
        M = len(ss) - 1
        ld = lambda v: np.ascontiguousarray(v, dtype=np.longdouble)
        t, t_prev, t_curr = ld(t), ld(t_prev), ld(t_curr)
        gyr, acc, bg, ba = _f64(gyr), _f64(acc), _f64(bg), _f64(ba)
        out = np.zeros((M, 142))
        lp = lambda v: v.ctypes.data_as(C.POINTER(C.c_longdouble))
        self.call("preintegrate", M, ss.ctypes.data_as(c_int32_p), lp(t), _dp(gyr), _dp(acc), lp(t_prev), lp(t_curr), _dp(bg), _dp(ba),
                  float(gyr_meas_cov), float(acc_meas_cov), _dp(out))
        return out

    def slide_window(self, d):
        """plba_slide_window: `d` as window.slide_delta() makes it — n_drop, the appended keyframes / IMU edges / landmarks / observations,
        optional drop masks and the new window's fixed flags.  Returns (point_map, line_map): each old landmark's new index or -1."""
        s, keep = make_slide(d)      # (`keep`: the arrays behind the struct's pointers stay alive until the call returns)
        pm = np.zeros(max(self.dims.get("Np", 0), 1), np.int32); lm = np.zeros(max(self.dims.get("Nl", 0), 1), np.int32)
        self.call("slide_window", C.byref(s), _ip(pm), _ip(lm))
        pm, lm = pm[:self.dims.get("Np", 0)], lm[:self.dims.get("Nl", 0)]
        sz = np.zeros(6, np.int32)
        self.call("get_sizes", _ip(sz))      # (the library merged the lists: its counts serve the getters)
        for k, v in zip(("K", "Np", "Nl", "Ep", "El", "M"), sz):
            self.dims[k] = int(v)
        return pm, lm

    # -- convenience -------------------------------------------------------------------------
    def upload_window(self, w):
        """Upload a synthetic window (window.make_window) following the reference's graph
        construction order (mapHandler.cpp:5799-6034)."""
        c = w["cam"]
        self.set_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["Rbc"], c["Pbc"])
        self.set_gravity(w["gw"])
        k = w["kf"]
        self.set_keyframes(k["vid_pvr"], k["vid_bias"], k["P"], k["V"], k["q"], k["bg"], k["ba"], k["dbg"], k["dba"],
                           k["fixed_pvr"], k["fixed_bias"])
        self.set_points(w["points"], w.get("point_fixed"))
        self.set_lines(w["lines"], w.get("line_fixed"))
        self.set_point_obs(w["po_pt"], w["po_kf"], w["po_uv"], w["po_w"])
        self.set_line_obs(w["lo_ln"], w["lo_kf"], w["lo_l"], w["lo_w"])
        if w.get("imu") is not None:
            im = w["imu"]
            self.set_imu_edges(im["kf_i"], im["kf_j"], im["preint"], im["info_pvr"], im["info_bias"])
        else:      # a handle keeps its arrays until they are set again: a window without IMU edges clears the previous window's
            self.set_imu_edges(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 142)), np.zeros((0, 81)), np.zeros((0, 36)))
        self.set_prior(w.get("prior"))
        for kind, d in w["huber"].items():
            self.set_robust(kind, True, d)
