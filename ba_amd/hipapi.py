"""ctypes binding of the C-ABI in include/ba_hip.h (ba_amd/lib/libba_hip.so).

The library is the product: if it is missing or no MI355X is usable this module fails
loudly — there is no CPU fallback anywhere in ba_amd.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libba_hip.so")
if os.environ.get("BA_AMD_LIB"):   # A/B measurements of library builds (scratch/): another libba_hip.so
    LIB_PATH = os.path.abspath(os.environ["BA_AMD_LIB"])

dp = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)


class Options(C.Structure):
    _fields_ = [("projection_outlier_threshold", C.c_double),
                ("use_robust_norm_for_proj_residuals", C.c_int32),
                ("use_robust_norm_for_inertial_residuals", C.c_int32),
                ("use_triangular_matrices", C.c_int32), ("keep_reduced_system", C.c_int32),
                ("gyro_sigma", C.c_double), ("accel_sigma", C.c_double),
                ("gyro_bias_sigma", C.c_double), ("accel_bias_sigma", C.c_double),
                ("pivot_rel_tolerance", C.c_double)]


class Errors(C.Structure):
    _fields_ = [("proj_error", C.c_double), ("binary_error", C.c_double),
                ("unary_error", C.c_double), ("inertial_error", C.c_double)]

    def total(self):
        return self.proj_error + self.binary_error + self.unary_error + self.inertial_error


class DoglegScalars(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("rhs_p_sq", "rhs_l_sq", "j_rhs_sq", "gn_p_sq",
                                          "gn_l_sq", "rhs_gn_p", "rhs_gn_l",
                                          "rhs_k_sq", "gn_k_sq", "rhs_gn_k")]


class StepNorms(C.Structure):
    _fields_ = [("step_p_norm", C.c_double), ("step_l_norm", C.c_double)]


class Timers(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("j_evaluation", "robust_weights", "jtj_schur", "solve",
                                          "back_substitution", "evaluate_residuals",
                                          "apply_update")]


class KernelStats(C.Structure):
    _fields_ = [("syrk_launches", C.c_uint32), ("gather_launches", C.c_uint32),
                ("landmarks_launches", C.c_uint32), ("imu_launches", C.c_uint32),
                ("syrk_ms", C.c_double), ("gather_ms", C.c_double), ("landmarks_ms", C.c_double),
                ("syrk_flops", C.c_double), ("imu_ms", C.c_double), ("pose_blocks_ms", C.c_double),
                ("pose_blocks_launches", C.c_uint32), ("reserved", C.c_uint32)]


class StructureStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("poses_active", "landmarks_active", "observations", "incidences",
                                          "factor_rows", "pair_blocks", "pair_entries", "tiles_lower",
                                          "tiles_S", "tiles_L", "tile_refs", "pose_entries", "linearize_waves",
                                          "factor_tile_products")]


class CommStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("chain_bytes_sent", "chain_bytes_recv", "side_bytes_sent", "side_bytes_recv",
                                          "reduce_scatter_bytes", "allreduce_bytes")] + \
               [(n, C.c_uint64) for n in ("chain_messages", "side_messages", "factorisations")]


class DistPlanStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("factor_bytes", "chain_recv_max", "chain_recv_total", "side_recv_max",
                                          "side_recv_total", "chain_sent_total", "side_sent_total", "recv_max",
                                          "backward_allreduce_bytes")] + \
               [(n, C.c_uint32) for n in ("messages_chain", "messages_side", "panels", "ranks", "classes", "kout")]


def dist_plan_stats(nblk, nz_lower, nranks, layout="auto", kout=0):
    """Byte accounting of the distributed solve's message plan (pure host: no device needed).
    nz_lower: (nblk, nblk) uint8 tile pattern of the factor, or None for a dense one."""
    out = DistPlanStats()
    ptr = None
    if nz_lower is not None:
        nz = np.ascontiguousarray(nz_lower, dtype=np.uint8)
        assert nz.shape == (nblk, nblk)
        ptr = nz.ctypes.data_as(C.POINTER(C.c_uint8))
    rc = lib().ba_hip_dist_plan_stats(int(nblk), ptr, int(nranks), layout.encode(), int(kout), C.byref(out))
    if rc != 0:
        raise ValueError("layout %r does not exist for %d ranks" % (layout, nranks))
    return {k: getattr(out, k) for k, _ in DistPlanStats._fields_}


class OrderingStats(C.Structure):
    _fields_ = [("mode", C.c_int32), ("candidate", C.c_int32), ("group_size", C.c_uint32), ("num_groups", C.c_uint32),
                ("tile_products_natural", C.c_uint64), ("tile_products_chosen", C.c_uint64),
                ("host_ms", C.c_double), ("device_ms", C.c_double)]


class MarginalStats(C.Structure):
    _fields_ = [("selinv_ms", C.c_double), ("landmark_ms", C.c_double), ("tile_products", C.c_uint64),
                ("factor_tile_products", C.c_uint64), ("store_bytes", C.c_double), ("store_tiles", C.c_uint32),
                ("levels", C.c_uint32)]


class JointMarginalStats(C.Structure):
    _fields_ = [("solve_ms", C.c_double), ("gram_ms", C.c_double), ("workspace_bytes", C.c_double),
                ("tile_products", C.c_uint64), ("columns", C.c_uint32), ("reach_tiles", C.c_uint32),
                ("levels", C.c_uint32), ("reserved", C.c_uint32)]


class JointStateStats(C.Structure):
    _fields_ = [("rhs_ms", C.c_double), ("seed_ms", C.c_double), ("incidences", C.c_uint64),
                ("landmark_columns", C.c_uint32), ("seed_tiles", C.c_uint32)]


class LeverageStats(C.Structure):
    _fields_ = [("device_ms", C.c_double), ("block_reads", C.c_uint64), ("residuals", C.c_uint32),
                ("landmarks", C.c_uint32)]


class PosePoseLeverageStats(C.Structure):
    _fields_ = [("device_ms", C.c_double), ("sigma_blocks", C.c_uint64), ("residuals", C.c_uint32),
                ("kind", C.c_uint32)]


JOINT_MAX_COLUMNS = 512  # BA_HIP_JOINT_MAX_COLUMNS


class FactorSolveStats(C.Structure):
    _fields_ = [("forward_ms", C.c_double), ("backward_ms", C.c_double), ("workspace_bytes", C.c_double),
                ("tile_products", C.c_uint64), ("columns", C.c_uint32), ("tiles", C.c_uint32),
                ("forward_levels", C.c_uint32), ("backward_levels", C.c_uint32)]


FACTOR_SOLVE_MAX_COLUMNS = 512  # BA_HIP_FACTOR_SOLVE_MAX_COLUMNS


class ModeOptions(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("max_iterations", C.c_uint32), ("seed", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class ModeStats(C.Structure):
    _fields_ = [("solve_ms", C.c_double), ("ortho_ms", C.c_double), ("residual_max", C.c_double),
                ("workspace_bytes", C.c_double), ("iterations", C.c_uint32), ("converged", C.c_uint32),
                ("block", C.c_uint32), ("reserved", C.c_uint32)]


class MarginalizationStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("blanket_poses", "absorbed_projection", "absorbed_unary", "absorbed_binary",
                                          "absorbed_inertial", "absorbed_priors", "dropped_projection", "reserved")] + \
               [("device_ms", C.c_double), ("host_ms", C.c_double)]


class PcgOptions(C.Structure):
    _fields_ = [("rel_tolerance", C.c_double), ("max_iterations", C.c_uint32), ("check_every", C.c_uint32),
                ("coarse_aggregate", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PcgStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("iterations", "converged", "residual_replacements", "breakdown")] + \
               [(n, C.c_double) for n in ("rel_residual_recurrence", "rel_residual_true", "rhs_norm", "solve_ms", "spmv_ms",
                                          "precond_ms")] + \
               [("tiles_read_per_spmv", C.c_uint64), ("bytes_read_per_spmv", C.c_double)]


class PcgCoarseStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("aggregate_used", "coarse_unknowns", "aggregates", "reserved")] + \
               [(n, C.c_double) for n in ("setup_ms", "apply_ms", "coarse_bytes")]


class PcgPanelStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("columns", "column_blocks", "passes", "converged", "capped", "broken_down")] + \
               [(n, C.c_double) for n in ("max_rel_residual_true", "solve_ms", "spmm_ms", "tile_products_per_pass",
                                          "bytes_read_per_product", "workspace_bytes")]


PCG_PANEL_MAX_COLUMNS = 512  # BA_HIP_PCG_PANEL_MAX_COLUMNS


class DampingTerms(C.Structure):
    """ba_hip_damping_terms"""
    _fields_ = [("lambda_", C.c_double), ("predicted_decrease", C.c_double), ("step_scaled_sq", C.c_double),
                ("diag_min", C.c_double), ("diag_max", C.c_double), ("device_ms", C.c_double)]


class TriangulationOptions(C.Structure):
    """ba_hip_triangulation_options, with the header's defaults"""
    _fields_ = [("linear_init", C.c_int32), ("max_iterations", C.c_int32), ("write_back", C.c_int32), ("reserved", C.c_int32),
                ("lambda0", C.c_double), ("gradient_tolerance", C.c_double), ("step_tolerance", C.c_double),
                ("min_parallax", C.c_double), ("huber_width", C.c_double)]

    def __init__(self, **kw):
        super().__init__(linear_init=1, max_iterations=20, write_back=1, lambda0=1e-3, gradient_tolerance=1e-6,
                         step_tolerance=1e-12, min_parallax=0.0, huber_width=0.0)
        for k, v in kw.items():
            if k not in dict(self._fields_) or k == "reserved":
                raise TypeError("unknown triangulation option %r" % k)
            setattr(self, k, v)


class TriangulationStats(C.Structure):
    """ba_hip_triangulation_stats"""
    _fields_ = [("count", C.c_uint32 * 6), ("landmarks", C.c_uint32), ("waves", C.c_uint32), ("waves_early", C.c_uint32),
                ("written", C.c_uint32), ("device_ms", C.c_double)]


# BA_HIP_TRI_*: the status of a result row of Engine.triangulate_landmarks
TRI_OK, TRI_NOT_CONVERGED, TRI_TOO_FEW_VIEWS, TRI_LOW_PARALLAX, TRI_BEHIND_CAMERA, TRI_FAILED = range(6)
TRI_STATUS_NAMES = ("OK", "NOT_CONVERGED", "TOO_FEW_VIEWS", "LOW_PARALLAX", "BEHIND_CAMERA", "FAILED")
# columns of a result row
TRI_STATUS, TRI_OBSERVATIONS, TRI_ITERATIONS, TRI_COST_START, TRI_COST_END, TRI_PARALLAX, TRI_MIN_DEPTH, TRI_GRADIENT = range(8)


class PoseRefinementOptions(C.Structure):
    """ba_hip_pose_refinement_options, with the header's defaults"""
    _fields_ = [("max_iterations", C.c_int32), ("write_back", C.c_int32), ("fixed_mask", C.c_uint32), ("reserved", C.c_int32),
                ("initial_damping", C.c_double), ("gradient_tolerance", C.c_double), ("step_tolerance", C.c_double),
                ("huber_width", C.c_double)]

    def __init__(self, **kw):
        super().__init__(max_iterations=20, write_back=1, fixed_mask=0, initial_damping=1e-3, gradient_tolerance=1e-6,
                         step_tolerance=1e-12, huber_width=0.0)
        for k, v in kw.items():
            if k not in dict(self._fields_) or k == "reserved":
                raise TypeError("unknown pose refinement option %r" % k)
            setattr(self, k, v)


class PoseRefinementStats(C.Structure):
    """ba_hip_pose_refinement_stats"""
    _fields_ = [("count", C.c_uint32 * 4), ("poses", C.c_uint32), ("written", C.c_uint32),
                ("observations_used", C.c_uint64), ("observations_excluded", C.c_uint64), ("device_ms", C.c_double)]


# BA_HIP_RESECT_*: the status of a result row of Engine.refine_poses
RESECT_OK, RESECT_NOT_CONVERGED, RESECT_TOO_FEW_OBSERVATIONS, RESECT_FAILED = range(4)
RESECT_STATUS_NAMES = ("OK", "NOT_CONVERGED", "TOO_FEW_OBSERVATIONS", "FAILED")
# columns of a result row
(RESECT_STATUS, RESECT_USED, RESECT_ITERATIONS, RESECT_COST_START, RESECT_COST_END, RESECT_MIN_DEPTH, RESECT_GRADIENT,
 RESECT_EXCLUDED) = range(8)


def _pcg_stats_dict(st):
    return {k: getattr(st, k) for k, _ in type(st)._fields_ if k != "reserved"}


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)
COLLECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int)

# every entry point include/ba_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "ba_hip_create", "ba_hip_destroy", "ba_hip_last_error", "ba_hip_set_options",
    "ba_hip_set_cameras", "ba_hip_set_pose_cam_params", "ba_hip_set_poses", "ba_hip_set_landmarks",
    "ba_hip_set_projection_residuals", "ba_hip_set_unary_residuals",
    "ba_hip_set_binary_residuals", "ba_hip_set_imu_residuals", "ba_hip_set_inertial_covariance_once", "ba_hip_set_imu_noise", "ba_hip_integrate_imu", "ba_hip_set_gravity",
    "ba_hip_finalize", "ba_hip_begin_solve", "ba_hip_set_pose_masks", "ba_hip_linearize",
    "ba_hip_solve_gn", "ba_hip_dogleg_terms", "ba_hip_compose_step", "ba_hip_apply_step",
    "ba_hip_rollback", "ba_hip_eval_residuals", "ba_hip_end_solve", "ba_hip_get_poses",
    "ba_hip_get_landmarks", "ba_hip_get_landmark_flags", "ba_hip_num_pose_params",
    "ba_hip_num_lm_params", "ba_hip_get_S", "ba_hip_get_rhs", "ba_hip_get_delta_gn",
    "ba_hip_get_step", "ba_hip_get_proj_weights", "ba_hip_get_proj_residuals", "ba_hip_get_imu_residuals", "ba_hip_get_imu_errors", "ba_hip_get_timers", "ba_hip_get_unary_scales", "ba_hip_device_buffer",
    "ba_hip_set_allreduce", "ba_hip_set_collectives", "ba_hip_solve_is_distributed", "ba_hip_dense_solve", "ba_hip_select_kth", "ba_hip_set_profiling",
    "ba_hip_get_kernel_stats", "ba_hip_check_solve", "ba_hip_get_structure_stats", "ba_hip_debug_set", "ba_hip_set_conditioning_residuals",
    "ba_hip_get_conditioning_error", "ba_hip_comm_unique_id", "ba_hip_comm_init", "ba_hip_comm_destroy", "ba_hip_allreduce_host", "ba_hip_get_proj_jacobians",
    "ba_hip_set_calibration", "ba_hip_num_calib_params", "ba_hip_get_cameras", "ba_hip_get_calib_jacobians", "ba_hip_get_calibration_marginals", "ba_hip_set_landmark_ref_pixels", "ba_hip_get_camera_params",
    "ba_hip_set_camera_models", "ba_hip_get_camera_fov",
    "ba_hip_integrate_imu_jacobians", "ba_hip_imu_pose_derivative", "ba_hip_imu_integrate_pose", "ba_hip_lie",
    "ba_hip_get_comm_stats", "ba_hip_reset_comm_stats", "ba_hip_dist_plan_stats", "ba_hip_get_factor_tile_pattern",
    "ba_hip_set_pose_ordering", "ba_hip_set_pose_permutation", "ba_hip_get_pose_ordering", "ba_hip_get_pose_group_graph",
    "ba_hip_compute_marginals", "ba_hip_get_pose_marginals", "ba_hip_get_pose_pair_marginals",
    "ba_hip_get_calibration_block_marginals", "ba_hip_get_landmark_marginals", "ba_hip_get_marginal_stats",
    "ba_hip_release_marginals", "ba_hip_get_joint_marginals", "ba_hip_get_joint_marginal_stats",
    "ba_hip_set_dense_priors", "ba_hip_get_prior_errors", "ba_hip_marginalize", "ba_hip_get_marginalization",
    "ba_hip_release_marginalization", "ba_hip_set_unary_scales",
    "ba_hip_set_reduced_solver", "ba_hip_get_pcg_stats", "ba_hip_pcg_solve", "ba_hip_tile_solve",
    "ba_hip_get_pcg_coarse_stats", "ba_hip_get_pcg_coarse",
    "ba_hip_get_projection_leverages", "ba_hip_get_leverage_stats", "ba_hip_device_bytes_live",
    "ba_hip_get_pose_pose_leverages", "ba_hip_get_pose_pose_leverage_stats", "ba_hip_num_pose_pose_residuals",
    "ba_hip_get_joint_state_marginals", "ba_hip_get_joint_state_stats",
    "ba_hip_factor_solve", "ba_hip_get_factor_solve_stats", "ba_hip_tile_factor_solve",
    "ba_hip_get_weakest_modes", "ba_hip_get_mode_stats",
    "ba_hip_pcg_panel_solve_system", "ba_hip_get_joint_marginals_pcg", "ba_hip_get_pcg_panel_stats",
    "ba_hip_get_pcg_panel_columns", "ba_hip_pcg_panel_solve",
    "ba_hip_set_damping", "ba_hip_get_damping_terms", "ba_hip_get_damping_diagonal",
    "ba_hip_damping_update",
    "ba_hip_triangulate_landmarks", "ba_hip_get_triangulation_stats",
    "ba_hip_refine_poses", "ba_hip_get_pose_refinement_stats",
]

ORDER_NATURAL, ORDER_AUTO, ORDER_USER = 0, 1, 2  # ba_hip_set_pose_ordering modes
SOLVER_DIRECT, SOLVER_PCG = 0, 1                 # ba_hip_set_reduced_solver modes
RES_UNARY, RES_BINARY, RES_IMU = 0, 1, 2         # BA_HIP_RES_*: kinds of ba_hip_get_pose_pose_leverages


def build(force=False):
    """Compile the gfx950 engine in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "clean", "-s"])
    subprocess.check_call(["make", "-C", src, "-j4", "-s"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "ba_amd: %s is missing — build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback"
                % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 /
        # libhsa-runtime64.  If the engine pulled in /opt/rocm's copies first, a later
        # `import torch` would bring a second HSA runtime into the process and torch would
        # see no GPU (measured on the MI355X box).  Importing torch first makes the engine
        # bind to torch's runtime (same SONAME), so torch.distributed/RCCL and the engine
        # share one device context.  C++ users without torch link /opt/rocm directly.
        try:
            import torch  # noqa: F401
        except Exception:  # torch absent: the engine uses the ROCm runtime it was linked with
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.ba_hip_last_error.restype = C.c_char_p
        _lib.ba_hip_num_pose_params.restype = C.c_uint32
        _lib.ba_hip_num_lm_params.restype = C.c_uint32
        _lib.ba_hip_num_calib_params.restype = C.c_uint32
        _lib.ba_hip_device_bytes_live.restype = C.c_uint64
        _lib.ba_hip_num_pose_pose_residuals.restype = C.c_uint32
    return _lib


class HipError(RuntimeError):
    pass


def device_bytes_live():
    """Device bytes held by the buffers of every live engine of this process (ba_hip_device_bytes_live)."""
    return int(lib().ba_hip_device_bytes_live())


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


class Engine:
    """Thin object wrapper of one ba_hip_engine (one device)."""

    def __init__(self, lm_dim=1, pose_dim=6, device=0, stream=None):
        self.L = lib()
        self.lm_dim, self.pose_dim = lm_dim, pose_dim
        self.num_poses = None   # recorded by set_poses; refine_poses(ids=None) needs it, or its num_poses argument
        self.h = C.c_void_p()
        rc = self.L.ba_hip_create(lm_dim, pose_dim, device, C.c_void_p(stream), C.byref(self.h))
        if rc != 0 or not self.h:
            raise HipError("ba_hip_create failed (rc=%d): no usable HIP device — "
                           "the engine has no CPU fallback" % rc)
        self._cb = None

    def close(self):
        if self.h:
            self.L.ba_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, positive_ok=False):
        if rc < 0 or (rc > 0 and not positive_ok):
            raise HipError("ba_hip call failed rc=%d: %s" %
                           (rc, self.L.ba_hip_last_error(self.h).decode()))
        return rc

    # -- upload ----------------------------------------------------------------
    def set_options(self, opt):
        self._chk(self.L.ba_hip_set_options(self.h, C.byref(opt)))

    def set_cameras(self, params, t_vs):
        """params: C x 4 (calibu::LinearCamera) or C x 5 (calibu::FovCamera: fx, fy, u0, v0, w)."""
        p = np.atleast_2d(_d(params))
        if p.shape[1] not in (4, 5):
            p = p.reshape(-1, 4)
        t = _d(t_vs).reshape(-1, 7)
        p4 = np.ascontiguousarray(p[:, :4])
        self._chk(self.L.ba_hip_set_cameras(self.h, p4.shape[0], _p(p4, dp), _p(t, dp)))
        if p.shape[1] == 5:
            self.set_camera_models(np.ones(p.shape[0], dtype=np.int32), p[:, 4])

    def set_camera_models(self, model, w):
        m, ww = np.ascontiguousarray(model, dtype=np.int32), _d(w)
        self._chk(self.L.ba_hip_set_camera_models(self.h, m.shape[0], m.ctypes.data_as(C.POINTER(C.c_int32)), _p(ww, dp)))

    def get_camera_fov(self, n):
        w = np.empty(n)
        self._chk(self.L.ba_hip_get_camera_fov(self.h, int(n), _p(w, dp)))
        return w

    def set_pose_cam_params(self, params):
        """P x 4 pinhole intrinsics per pose (use_per_pose_cam_params), None = rig camera."""
        if params is None:
            self._chk(self.L.ba_hip_set_pose_cam_params(self.h, 0, None))
        else:
            p = _d(params).reshape(-1, 4)
            self._chk(self.L.ba_hip_set_pose_cam_params(self.h, p.shape[0], _p(p, dp)))

    def set_poses(self, t_wp, v_w=None, b=None, is_active=None):
        t = _d(t_wp).reshape(-1, 7)
        v = _d(v_w) if v_w is not None else None
        bb = _d(b) if b is not None else None
        a = np.ascontiguousarray(is_active, dtype=np.uint8) if is_active is not None else None
        self.num_poses = t.shape[0]
        self._chk(self.L.ba_hip_set_poses(self.h, t.shape[0], _p(t, dp), _p(v, dp), _p(bb, dp),
                                          _p(a, u8p)))

    def set_landmarks(self, x_w, ref_pose, ref_cam=None, is_active=None):
        x = _d(x_w).reshape(-1, 4)
        rp = np.ascontiguousarray(ref_pose, dtype=np.uint32)
        rc = np.ascontiguousarray(ref_cam, dtype=np.uint32) if ref_cam is not None else None
        a = np.ascontiguousarray(is_active, dtype=np.uint8) if is_active is not None else None
        self.num_landmarks = x.shape[0]
        self._chk(self.L.ba_hip_set_landmarks(self.h, x.shape[0], _p(x, dp), _p(rp, u32p),
                                              _p(rc, u32p), _p(a, u8p)))

    def set_projection_residuals(self, z, pose, lm, cam=None, weight=None):
        zz = _d(z).reshape(-1, 2)
        pp = np.ascontiguousarray(pose, dtype=np.uint32)
        ll = np.ascontiguousarray(lm, dtype=np.uint32)
        cc = np.ascontiguousarray(cam, dtype=np.uint32) if cam is not None else None
        ww = _d(weight) if weight is not None else None
        self._chk(self.L.ba_hip_set_projection_residuals(self.h, zz.shape[0], _p(zz, dp),
                                                         _p(pp, u32p), _p(ll, u32p), _p(cc, u32p),
                                                         _p(ww, dp)))

    def finalize(self):
        self._chk(self.L.ba_hip_finalize(self.h))

    # -- phases ----------------------------------------------------------------
    def begin_solve(self):
        self._chk(self.L.ba_hip_begin_solve(self.h))

    def set_pose_masks(self, masks):
        m = np.ascontiguousarray(masks, dtype=np.uint16)
        self._chk(self.L.ba_hip_set_pose_masks(self.h, m.shape[0], _p(m, u16p)))

    def linearize(self):
        e = Errors()
        self._chk(self.L.ba_hip_linearize(self.h, C.byref(e)))
        return e

    def solve_gn(self):
        return self._chk(self.L.ba_hip_solve_gn(self.h), positive_ok=True)

    def dogleg_terms(self, gn_available):
        s = DoglegScalars()
        self._chk(self.L.ba_hip_dogleg_terms(self.h, int(gn_available), C.byref(s)))
        return s

    def set_damping(self, lam):
        """Levenberg-Marquardt damping of the next linearize(): (H + lam diag(d)) delta = g; 0 = off."""
        self._chk(self.L.ba_hip_set_damping(self.h, C.c_double(lam)))

    def damping_terms(self):
        """dict of ba_hip_damping_terms: lambda of the held linearisation, predicted_decrease and step_scaled_sq of the
        last solve_gn, diag_min / diag_max of the damping diagonal, device_ms of the damping kernels."""
        t = DampingTerms()
        self._chk(self.L.ba_hip_get_damping_terms(self.h, C.byref(t)))
        return {"lambda": t.lambda_, "predicted_decrease": t.predicted_decrease, "step_scaled_sq": t.step_scaled_sq,
                "diag_min": t.diag_min, "diag_max": t.diag_max, "device_ms": t.device_ms}

    def damping_diagonal(self):
        """(d_p, d_l) of the damped linearisation: pose rows in the caller's order, landmarks by optimisation index."""
        n, nl = self.num_pose_params(), self.num_lm_params()
        a, c = np.zeros(max(n, 1)), np.zeros(max(nl, 1))
        self._chk(self.L.ba_hip_get_damping_diagonal(self.h, _p(a, dp), _p(c, dp)))
        return a[:n], c[:nl]

    def triangulate_landmarks(self, ids=None, **options):
        """Closed-form triangulation and per-landmark Levenberg-Marquardt refinement with the poses held fixed
        (ba_hip_triangulate_landmarks); outside a Solve.  ids: landmark ids, each once, None = every landmark.  options:
        the fields of TriangulationOptions.  Returns (results n x 8, x_w n x 4): per landmark the status TRI_*, observations,
        iterations, cost at the start and the end, parallax, smallest depth, gradient measure; and the world coordinates
        the call arrived at where it accepts them, the coordinates held elsewhere."""
        o = TriangulationOptions(**options)
        if ids is None:
            n, idp = getattr(self, "num_landmarks", 0), None
        else:
            ida = np.ascontiguousarray(ids, dtype=np.uint32)
            n, idp = ida.shape[0], _p(ida, u32p)
        res, xw = np.zeros((max(n, 1), 8)), np.zeros((max(n, 1), 4))
        self._chk(self.L.ba_hip_triangulate_landmarks(self.h, n, idp, C.byref(o), _p(res, dp), _p(xw, dp)))
        return res[:n], xw[:n]

    def triangulation_stats(self):
        """dict of ba_hip_triangulation_stats of the last triangulate_landmarks: count per status name, landmarks, waves,
        waves_early, written, device_ms."""
        t = TriangulationStats()
        self._chk(self.L.ba_hip_get_triangulation_stats(self.h, C.byref(t)))
        return {"count": {TRI_STATUS_NAMES[i]: int(t.count[i]) for i in range(6)}, "landmarks": t.landmarks, "waves": t.waves,
                "waves_early": t.waves_early, "written": t.written, "device_ms": t.device_ms}

    def refine_poses(self, ids=None, num_poses=None, **options):
        """Per-pose Levenberg-Marquardt refinement (resection) with the landmarks held fixed (ba_hip_refine_poses);
        outside a Solve.  ids: pose ids, each once, None = every pose (num_poses: their count, for an Engine that did not
        upload the poses itself; set_poses records it otherwise).  options: the fields of PoseRefinementOptions.
        Returns (results n x 8, t_wp n x 7, info n x 6 x 6): per pose the status RESECT_*, observations used, iterations,
        cost at the start and the end, smallest depth, gradient measure, observations excluded; the pose (t, q xyzw) the
        call arrived at where it accepts it, the pose held elsewhere; the undamped H at the end point."""
        o = PoseRefinementOptions(**options)
        if ids is None:
            n, idp = getattr(self, "num_poses", None) if num_poses is None else int(num_poses), None
            if n is None:
                raise ValueError("refine_poses: this Engine did not upload the poses itself, pass ids or num_poses")
        else:
            ida = np.ascontiguousarray(ids, dtype=np.uint32)
            n, idp = ida.shape[0], _p(ida, u32p)
        res, t7, info = np.zeros((max(n, 1), 8)), np.zeros((max(n, 1), 7)), np.zeros((max(n, 1), 6, 6))
        self._chk(self.L.ba_hip_refine_poses(self.h, n, idp, C.byref(o), _p(res, dp), _p(t7, dp), _p(info, dp)))
        return res[:n], t7[:n], info[:n]

    def pose_refinement_stats(self):
        """dict of ba_hip_pose_refinement_stats of the last refine_poses: count per status name, poses, written,
        observations_used, observations_excluded, device_ms."""
        t = PoseRefinementStats()
        self._chk(self.L.ba_hip_get_pose_refinement_stats(self.h, C.byref(t)))
        return {"count": {RESECT_STATUS_NAMES[i]: int(t.count[i]) for i in range(4)}, "poses": t.poses, "written": t.written,
                "observations_used": t.observations_used, "observations_excluded": t.observations_excluded,
                "device_ms": t.device_ms}

    def compose_step(self, coef_rhs, coef_gn):
        n = StepNorms()
        self._chk(self.L.ba_hip_compose_step(self.h, C.c_double(coef_rhs), C.c_double(coef_gn),
                                             C.byref(n)))
        return n

    def apply_step(self):
        self._chk(self.L.ba_hip_apply_step(self.h))

    def rollback(self):
        self._chk(self.L.ba_hip_rollback(self.h))

    def eval_residuals(self):
        e = Errors()
        self._chk(self.L.ba_hip_eval_residuals(self.h, C.byref(e)))
        return e

    def end_solve(self):
        self._chk(self.L.ba_hip_end_solve(self.h))

    # -- results -----------------------------------------------------------------
    def num_pose_params(self):
        return self.L.ba_hip_num_pose_params(self.h)

    def num_lm_params(self):
        return self.L.ba_hip_num_lm_params(self.h)

    def get_poses(self, n):
        t, v, b = np.empty((n, 7)), np.empty((n, 3)), np.empty((n, 6))
        self._chk(self.L.ba_hip_get_poses(self.h, _p(t, dp), _p(v, dp), _p(b, dp)))
        return t, v, b

    def get_landmarks(self, n):
        x = np.empty((n, 4))
        self._chk(self.L.ba_hip_get_landmarks(self.h, _p(x, dp)))
        return x

    def get_landmark_flags(self, n):
        r, o = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint32)
        self._chk(self.L.ba_hip_get_landmark_flags(self.h, _p(r, u8p), _p(o, u32p)))
        return r, o

    def num_calib_params(self):
        return self.L.ba_hip_num_calib_params(self.h)

    def set_calibration(self, calib_size=0, do_tvs=True):
        """CalibSize / DoTvs of the reference's class template; before finalize()."""
        self._chk(self.L.ba_hip_set_calibration(self.h, int(calib_size), int(do_tvs)))

    def get_calibration_marginals(self):
        k = self.num_calib_params()
        c = np.empty((k, k))
        self._chk(self.L.ba_hip_get_calibration_marginals(self.h, _p(c, dp)))
        return c

    # ---- marginal covariances (selected inverse of the last factor; ba_hip.h) ----
    def compute_marginals(self):
        self._chk(self.L.ba_hip_compute_marginals(self.h))

    def pose_marginals(self, ids):
        """(n, D, D) covariances of the poses `ids` (caller's pose ids)."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32)
        D = self.pose_dim
        out = np.empty((len(ids), D, D))
        self._chk(self.L.ba_hip_get_pose_marginals(self.h, len(ids), _p(ids, u32p), _p(out, dp)))
        return out

    def pose_pair_marginals(self, a, b):
        """(n, D, D) cross covariances Cov(a_i, b_i)."""
        a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.uint32)
        b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.uint32)
        if a.shape != b.shape:
            raise ValueError("pose_pair_marginals: a and b differ in length")
        D = self.pose_dim
        out = np.empty((len(a), D, D))
        self._chk(self.L.ba_hip_get_pose_pair_marginals(self.h, len(a), _p(a, u32p), _p(b, u32p), _p(out, dp)))
        return out

    def calibration_block_marginals(self):
        """K x K calibration block read from the selected inverse."""
        k = self.num_calib_params()
        c = np.empty((k, k))
        self._chk(self.L.ba_hip_get_calibration_block_marginals(self.h, _p(c, dp)))
        return c

    def landmark_marginals(self, ids=None):
        """(n, LM, LM) landmark covariances; ids=None: every active landmark by optimisation index."""
        lm = self.lm_dim
        if ids is None:
            n = self.num_lm_params() // max(lm, 1)
            out = np.empty((n, lm, lm))
            self._chk(self.L.ba_hip_get_landmark_marginals(self.h, n, None, _p(out, dp)))
            return out
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32)
        out = np.empty((len(ids), lm, lm))
        self._chk(self.L.ba_hip_get_landmark_marginals(self.h, len(ids), _p(ids, u32p), _p(out, dp)))
        return out

    def marginal_stats(self):
        st = MarginalStats()
        self._chk(self.L.ba_hip_get_marginal_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in MarginalStats._fields_}

    def release_marginals(self):
        self._chk(self.L.ba_hip_release_marginals(self.h))

    # ---- leverages of projection residuals (hat blocks; ba_hip.h) ----
    def projection_leverages(self, ids=None, count=None):
        """(n, 2, 2) blocks H_aa of the hat matrix per accepted projection residual id; ids=None: every residual in
        residual-id order (count: their number, default the engine's)."""
        if ids is None:
            n = int(self.structure_stats()["observations"]) if count is None else int(count)
            out = np.empty((n, 2, 2))
            self._chk(self.L.ba_hip_get_projection_leverages(self.h, n, None, _p(out, dp)))
            return out
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32).ravel()
        out = np.empty((len(ids), 2, 2))
        self._chk(self.L.ba_hip_get_projection_leverages(self.h, len(ids), _p(ids, u32p), _p(out, dp)))
        return out

    def leverage_stats(self):
        st = LeverageStats()
        self._chk(self.L.ba_hip_get_leverage_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in LeverageStats._fields_}

    # ---- leverages of unary, binary and inertial residuals (hat blocks; ba_hip.h) ----
    def pose_pose_leverages(self, kind, ids=None, count=None, want=(True, True, True)):
        """(cov, info, leverage) = ((n, 15, 15), (n, 15, 15), (n,)) of the residuals `ids` of `kind` (RES_UNARY,
        RES_BINARY, RES_IMU): C = J Sigma J^T in the residual's raw coordinates, the effective information Lambda,
        tr(C Lambda).  ids=None: every residual of the kind in id order (count: their number, default the
        engine's).  want: which of the three outputs to ask for (None in place of the others)."""
        if ids is None:
            n = int(self.L.ba_hip_num_pose_pose_residuals(self.h, int(kind))) if count is None else int(count)
            idp = None
        else:
            ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32).ravel()
            n, idp = len(ids), _p(ids, u32p)
        cov = np.empty((n, 15, 15)) if want[0] else None
        info = np.empty((n, 15, 15)) if want[1] else None
        lev = np.empty(n) if want[2] else None
        self._chk(self.L.ba_hip_get_pose_pose_leverages(self.h, int(kind), n, idp, _p(cov, dp), _p(info, dp), _p(lev, dp)))
        return cov, info, lev

    def pose_pose_leverage_stats(self):
        st = PosePoseLeverageStats()
        self._chk(self.L.ba_hip_get_pose_pose_leverage_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in PosePoseLeverageStats._fields_}

    # ---- joint covariance of a pose set (forward substitution + Gram product, no selected inverse) ----
    def joint_marginals(self, ids, include_calibration=False):
        """(M, M) joint covariance of the poses `ids` in the caller's order, the calibration rows last when asked
        for; M = len(ids) * D (+ K).  Any active poses, coupled by the factor's pattern or not."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32).ravel()
        m = len(ids) * self.pose_dim + (self.num_calib_params() if include_calibration else 0)
        out = np.empty((m, m))
        self._chk(self.L.ba_hip_get_joint_marginals(self.h, len(ids), _p(ids, u32p), int(bool(include_calibration)),
                                                    _p(out, dp)))
        return out

    def joint_marginal_stats(self):
        st = JointMarginalStats()
        self._chk(self.L.ba_hip_get_joint_marginal_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in JointMarginalStats._fields_ if k != "reserved"}

    # ---- solves with the kept factor: X = S^-1 B for the caller's right-hand sides ----
    def factor_solve(self, B):
        """X = S^-1 B with the factor the last direct solve_gn left: B is (n,) or (n, m), n = pose + calibration
        parameters, rows in the order of get_delta_gn; X has B's shape."""
        B = _d(B)
        n = self.num_pose_params() + self.num_calib_params()
        if B.ndim not in (1, 2) or B.shape[0] != n:
            raise ValueError("B must have %d rows" % n)
        m = 1 if B.ndim == 1 else B.shape[1]
        X = np.empty_like(B)
        self._chk(self.L.ba_hip_factor_solve(self.h, m, _p(B, dp), _p(X, dp)))
        return X

    def factor_solve_stats(self):
        st = FactorSolveStats()
        self._chk(self.L.ba_hip_get_factor_solve_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in FactorSolveStats._fields_}

    # ---- weakest modes: the eigenpairs of S of smallest magnitude, from the kept factor ----
    def weakest_modes(self, k, tolerance=None, max_iterations=None, seed=None):
        """(eigenvalues (k,), modes (k, n)): the k eigenpairs of the factorised S of smallest magnitude, ascending in
        magnitude; each mode is a unit vector over the rows of get_delta_gn.  None takes the engine's defaults
        (1e-8, 50 iterations, seed 1); when the cap is reached the last Ritz pairs come back and mode_stats() shows
        converged < k."""
        n = self.num_pose_params() + self.num_calib_params()
        lam, modes = np.zeros(int(k)), np.zeros((int(k), n))
        o = None
        if tolerance is not None or max_iterations is not None or seed is not None:
            o = C.byref(ModeOptions(float(tolerance or 0.0), int(max_iterations or 0), int(seed or 0)))
        self._chk(self.L.ba_hip_get_weakest_modes(self.h, int(k), o, _p(lam, dp), _p(modes, dp)))
        return lam, modes

    def mode_stats(self):
        st = ModeStats()
        self._chk(self.L.ba_hip_get_mode_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in ModeStats._fields_ if k != "reserved"}

    # ---- joint covariance of poses, calibration and landmarks (the cross blocks included) ----
    def joint_state_marginals(self, pose_ids, lm_ids, include_calibration=False):
        """(M, M) block of the inverse of the full system over the poses `pose_ids`, the calibration rows when asked
        for, and the landmarks `lm_ids`, columns in that order; M = len(pose_ids) * D (+ K) + len(lm_ids) * LmSize."""
        pose_ids = np.ascontiguousarray(np.atleast_1d(pose_ids), dtype=np.uint32).ravel()
        lm_ids = np.ascontiguousarray(np.atleast_1d(lm_ids), dtype=np.uint32).ravel()
        m = len(pose_ids) * self.pose_dim + (self.num_calib_params() if include_calibration else 0) + \
            len(lm_ids) * self.lm_dim
        out = np.empty((m, m))
        self._chk(self.L.ba_hip_get_joint_state_marginals(self.h, len(pose_ids), _p(pose_ids, u32p),
                                                          int(bool(include_calibration)), len(lm_ids), _p(lm_ids, u32p),
                                                          _p(out, dp)))
        return out

    def joint_state_stats(self):
        st = JointStateStats()
        self._chk(self.L.ba_hip_get_joint_state_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in JointStateStats._fields_}

    # ---- dense pose priors and marginalisation (ba_hip.h) ----
    def set_dense_priors(self, priors):
        """priors: list of dicts with pose_ids (k), x0 (k x 16), H (kD x kD), b (kD), c; before finalize."""
        D = self.pose_dim
        ptr = np.zeros(len(priors) + 1, dtype=np.uint32)
        for q, p in enumerate(priors):
            ptr[q + 1] = ptr[q] + len(p["pose_ids"])
        cat = lambda key, shape: (np.ascontiguousarray(np.concatenate([np.asarray(p[key], dtype=np.float64).reshape(shape)
                                                                       for p in priors]))
                                  if priors else np.zeros(1))
        ids = (np.ascontiguousarray(np.concatenate([np.asarray(p["pose_ids"], dtype=np.uint32) for p in priors]))
               if priors else np.zeros(1, dtype=np.uint32))
        x0 = cat("x0", (-1,))
        H = cat("H", (-1,))
        b = cat("b", (-1,))
        c = np.ascontiguousarray([float(p["c"]) for p in priors] or [0.0])
        for p in priors:
            k = len(p["pose_ids"])
            assert np.asarray(p["x0"]).size == 16 * k and np.asarray(p["H"]).size == (k * D) ** 2
        self._chk(self.L.ba_hip_set_dense_priors(self.h, len(priors), _p(ptr, u32p), _p(ids, u32p), _p(x0, dp), _p(H, dp),
                                                 _p(b, dp), _p(c, dp)))

    def prior_errors(self, n):
        out = np.zeros(max(n, 1))
        self._chk(self.L.ba_hip_get_prior_errors(self.h, n, _p(out, dp)))
        return out[:n]

    def marginalize(self, pose_ids, lm_ids=()):
        """ba_hip_marginalize + ba_hip_get_marginalization: a dict with pose_ids (the blanket), x0, H, b, c and the
        statistics.  Raises HipError on a refusal (a non-PD S^a_MM included)."""
        m = np.ascontiguousarray(pose_ids, dtype=np.uint32)
        l = np.ascontiguousarray(lm_ids, dtype=np.uint32)
        st = MarginalizationStats()
        self._chk(self.L.ba_hip_marginalize(self.h, len(m), _p(m, u32p) if len(m) else None, len(l),
                                            _p(l, u32p) if len(l) else None, C.byref(st)))
        nb, D = st.blanket_poses, self.pose_dim
        ids = np.zeros(max(nb, 1), dtype=np.uint32)
        x0 = np.zeros((max(nb, 1), 16))
        H = np.zeros((max(nb * D, 1), max(nb * D, 1)))
        b = np.zeros(max(nb * D, 1))
        c = C.c_double(0.0)
        self._chk(self.L.ba_hip_get_marginalization(self.h, _p(ids, u32p), _p(x0, dp), _p(H, dp), _p(b, dp), C.byref(c)))
        out = {"pose_ids": ids[:nb], "x0": x0[:nb], "H": H[:nb * D, :nb * D], "b": b[:nb * D], "c": c.value}
        out.update({k: getattr(st, k) for k, _ in MarginalizationStats._fields_ if k != "reserved"})
        return out

    def release_marginalization(self):
        self._chk(self.L.ba_hip_release_marginalization(self.h))

    def set_landmark_ref_pixels(self, z_ref):
        z = _d(z_ref).reshape(-1, 2)
        self._chk(self.L.ba_hip_set_landmark_ref_pixels(self.h, z.shape[0], _p(z, dp)))

    def get_camera_params(self, n):
        p = np.empty((n, 4))
        self._chk(self.L.ba_hip_get_camera_params(self.h, int(n), _p(p, dp)))
        return p

    def get_cameras(self, n):
        t = np.empty((n, 7))
        self._chk(self.L.ba_hip_get_cameras(self.h, int(n), _p(t, dp)))
        return t

    def get_calib_jacobians(self, n):
        """sqrt(w) dz_dtvs (2x6) per residual id of the last linearisation."""
        j = np.empty((n, 2, 6))
        self._chk(self.L.ba_hip_get_calib_jacobians(self.h, _p(j, dp)))
        return j

    def get_S(self):
        """(n + K)^2 with K calibration unknowns behind the n pose unknowns."""
        n = self.num_pose_params() + self.num_calib_params()
        s = np.empty((n, n))
        self._chk(self.L.ba_hip_get_S(self.h, _p(s, dp)))
        return s

    def get_rhs(self):
        n, nl = self.num_pose_params() + self.num_calib_params(), self.num_lm_params()
        a, b, c = np.empty(n), np.empty(n), np.zeros(max(nl, 1))
        self._chk(self.L.ba_hip_get_rhs(self.h, _p(a, dp), _p(b, dp), _p(c, dp)))
        return a, b, c[:nl]

    def get_delta_gn(self):
        n, nl = self.num_pose_params() + self.num_calib_params(), self.num_lm_params()
        a, c = np.empty(n), np.zeros(max(nl, 1))
        self._chk(self.L.ba_hip_get_delta_gn(self.h, _p(a, dp), _p(c, dp)))
        return a, c[:nl]

    def get_step(self):
        n, nl = self.num_pose_params() + self.num_calib_params(), self.num_lm_params()
        a, c = np.empty(n), np.zeros(max(nl, 1))
        self._chk(self.L.ba_hip_get_step(self.h, _p(a, dp), _p(c, dp)))
        return a, c[:nl]

    def get_proj_weights(self, n):
        w = np.empty(n)
        self._chk(self.L.ba_hip_get_proj_weights(self.h, _p(w, dp)))
        return w

    def get_proj_jacobians(self, n):
        """sqrt(w)-weighted (dz_dx_meas, dz_dx_ref, dz_dlm, r) per residual id of the last linearisation."""
        lm = max(self.lm_dim, 1)
        jm, jr, jl, r = np.zeros((n, 2, 6)), np.zeros((n, 2, 6)), np.zeros((n, 2, lm)), np.zeros((n, 2))
        self._chk(self.L.ba_hip_get_proj_jacobians(self.h, _p(jm, dp), _p(jr, dp), _p(jl, dp), _p(r, dp)))
        return jm, jr, jl[:, :, :self.lm_dim], r

    def get_timers(self):
        t = Timers()
        self._chk(self.L.ba_hip_get_timers(self.h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in Timers._fields_}

    def check_solve(self):
        """(|S delta_gn - rhs|, |rhs|) formed on the device from the kept copy of S."""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.ba_hip_check_solve(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def structure_stats(self):
        st = StructureStats()
        self._chk(self.L.ba_hip_get_structure_stats(self.h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in StructureStats._fields_}

    def set_pose_ordering(self, mode):
        """ORDER_NATURAL / ORDER_AUTO / ORDER_USER, effective at the next finalize()."""
        self._chk(self.L.ba_hip_set_pose_ordering(self.h, int(mode)))

    def set_pose_permutation(self, opt_of_natural):
        """The permutation of ORDER_USER: opt_of_natural[i] = factorised position of the i-th active pose."""
        p = np.ascontiguousarray(opt_of_natural, dtype=np.uint32)
        self._chk(self.L.ba_hip_set_pose_permutation(self.h, _p(p, u32p), len(p)))

    def get_pose_ordering(self):
        """(opt_of_natural, stats dict) of the last finalize."""
        n = self.num_pose_params() // self.pose_dim
        perm = np.zeros(max(n, 1), dtype=np.uint32)
        st = OrderingStats()
        self._chk(self.L.ba_hip_get_pose_ordering(self.h, _p(perm, u32p), C.byref(st)))
        return perm[:n], {k: getattr(st, k) for k, _ in OrderingStats._fields_}

    def get_pose_group_graph(self):
        """(ptr, adj) CSR of the group graph the last AUTO ordering was chosen from."""
        ng, ne = C.c_uint32(), C.c_uint32()
        self._chk(self.L.ba_hip_get_pose_group_graph(self.h, None, None, C.byref(ng), C.byref(ne)))
        ptr = np.zeros(ng.value + 1, dtype=np.uint32)
        adj = np.zeros(max(ne.value, 1), dtype=np.uint32)
        self._chk(self.L.ba_hip_get_pose_group_graph(self.h, _p(ptr, u32p), _p(adj, u32p), C.byref(ng), C.byref(ne)))
        return (ptr if ng.value else np.zeros(0, dtype=np.uint32)), adj[:ne.value]

    def debug_set(self, key, value):
        self._chk(self.L.ba_hip_debug_set(self.h, int(key), int(value)))

    def set_profiling(self, on):
        self._chk(self.L.ba_hip_set_profiling(self.h, int(on)))

    def kernel_stats(self):
        k = KernelStats()
        self._chk(self.L.ba_hip_get_kernel_stats(self.h, C.byref(k)))
        return k

    def set_allreduce(self, fn, rank, nranks):
        """fn(dev_ptr:int, count:int, dtype:int) -> int (0 = ok); kept alive by this object."""
        if fn is None:
            self._cb = None
            self._chk(self.L.ba_hip_set_allreduce(self.h, None, None, 0, 1))
            return
        self._cb = ALLREDUCE_FN(lambda ctx, ptr, count, dtype: int(fn(ptr, count, dtype)))
        self._chk(self.L.ba_hip_set_allreduce(self.h, self._cb, None, int(rank), int(nranks)))

    def set_collectives(self, fn):
        """fn(op:int, dev_ptr:int, count:int, root:int) -> int (0 = ok); op 1 = broadcast from
        root, op 2 = in-place reduce-scatter of nranks chunks of `count` doubles.  Switches the
        reduced solve from replicated to distributed (ba_hip.h: ba_hip_set_collectives)."""
        if fn is None:
            self._cb2 = None
            self._chk(self.L.ba_hip_set_collectives(self.h, None, None))
            return
        self._cb2 = COLLECTIVE_FN(lambda ctx, op, ptr, count, root: int(fn(op, ptr, count, root)))
        self._chk(self.L.ba_hip_set_collectives(self.h, self._cb2, None))

    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id (rank 0 creates it, the other ranks receive it out of band)."""
        buf = C.create_string_buffer(128)
        if lib().ba_hip_comm_unique_id(buf) != 0:
            raise HipError("ba_hip_comm_unique_id failed (librccl not loadable?)")
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        """Native RCCL communicator inside the engine (collective over all ranks)."""
        self._chk(self.L.ba_hip_comm_init(self.h, C.c_char_p(unique_id), int(rank), int(nranks)))

    def comm_destroy(self):
        self._chk(self.L.ba_hip_comm_destroy(self.h))

    def solve_is_distributed(self):
        return bool(self.L.ba_hip_solve_is_distributed(self.h))

    def comm_stats(self, reset=False):
        """Bytes this rank moved per stream of the communicator(s) since the last reset (ba_hip_comm_stats)."""
        out = CommStats()
        self._chk(self.L.ba_hip_get_comm_stats(self.h, C.byref(out)))
        if reset:
            self._chk(self.L.ba_hip_reset_comm_stats(self.h))
        return {k: getattr(out, k) for k, _ in CommStats._fields_}

    def factor_tile_pattern(self):
        """(nblk, nblk) uint8 lower tile pattern of the factor of the reduced system."""
        nblk = (self.num_pose_params() + self.num_calib_params() + 63) // 64
        nblk = max(nblk, 1)
        out = np.zeros((nblk, nblk), dtype=np.uint8)
        self._chk(self.L.ba_hip_get_factor_tile_pattern(self.h, nblk, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def set_reduced_solver(self, mode, rel_tolerance=1e-6, max_iterations=0, check_every=0, coarse_aggregate=0):
        """SOLVER_DIRECT (tile-sparse LDL^T, the default) or SOLVER_PCG (block-Jacobi preconditioned conjugate
        gradients on S; coarse_aggregate = g >= 1 adds the coarse-space correction over aggregates of g poses) for the
        following solve_gn calls; not structural, no finalize needed."""
        if int(mode) == SOLVER_DIRECT:
            self._chk(self.L.ba_hip_set_reduced_solver(self.h, SOLVER_DIRECT, None))
            return
        o = PcgOptions(float(rel_tolerance), int(max_iterations), int(check_every), int(coarse_aggregate))
        self._chk(self.L.ba_hip_set_reduced_solver(self.h, int(mode), C.byref(o)))

    def pcg_stats(self):
        """Statistics of the last solve_gn (a dict of ba_hip_pcg_stats); HipError if that solve was direct."""
        st = PcgStats()
        self._chk(self.L.ba_hip_get_pcg_stats(self.h, C.byref(st)))
        return _pcg_stats_dict(st)

    def pcg_coarse_stats(self):
        """ba_hip_pcg_coarse_stats of the last solve_gn / pcg_solve as a dict; HipError if it did not use the coarse space."""
        st = PcgCoarseStats()
        self._chk(self.L.ba_hip_get_pcg_coarse_stats(self.h, C.byref(st)))
        return _pcg_stats_dict(st)

    def pcg_coarse(self):
        """(C, C^-1) of the last two-level solve, nc x nc each."""
        nc = self.pcg_coarse_stats()["coarse_unknowns"]
        c, ci = np.empty((nc, nc)), np.empty((nc, nc))
        self._chk(self.L.ba_hip_get_pcg_coarse(self.h, nc, _p(c, dp), _p(ci, dp)))
        return c, ci

    def pcg_solve(self, a_lower, b, block, rel_tolerance, max_iterations=0, check_every=0, coarse_aggregate=0):
        """Stand-alone PCG on an SPD system given by its lower triangle: (x, rc, stats dict)."""
        a, b = _d(a_lower), _d(b)
        x = np.zeros(b.shape[0])
        o = PcgOptions(float(rel_tolerance), int(max_iterations), int(check_every), int(coarse_aggregate))
        st = PcgStats()
        rc = self._chk(self.L.ba_hip_pcg_solve(self.h, b.shape[0], _p(a, dp), _p(b, dp), int(block), C.byref(o), _p(x, dp),
                                               C.byref(st)), positive_ok=True)
        return x, rc, _pcg_stats_dict(st)

    # ---- panel PCG: S^-1 on a block of columns after a PCG solve (no factor) ----
    def pcg_panel_solve_system(self, B, rel_tolerance=1e-8, max_iterations=0, check_every=0, coarse_aggregate=0):
        """(X, rc): X = S^-1 B by the panel PCG after a PCG solve_gn; B is (n,) or (n, m), rows in the order of
        get_delta_gn.  rc is 0 or 4 (some column broke down: pcg_panel_columns names it)."""
        B = _d(B)
        n = self.num_pose_params() + self.num_calib_params()
        if B.ndim not in (1, 2) or B.shape[0] != n:
            raise ValueError("B must have %d rows" % n)
        m = 1 if B.ndim == 1 else B.shape[1]
        X = np.zeros_like(B)
        o = PcgOptions(float(rel_tolerance), int(max_iterations), int(check_every), int(coarse_aggregate))
        rc = self._chk(self.L.ba_hip_pcg_panel_solve_system(self.h, m, _p(B, dp), _p(X, dp), C.byref(o)), positive_ok=True)
        return X, rc

    def joint_marginals_pcg(self, ids, include_calibration=False, rel_tolerance=1e-8, max_iterations=0, check_every=0,
                            coarse_aggregate=0):
        """The block of joint_marginals without a factor: the panel PCG on unit columns, symmetrised."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32).ravel()
        m = len(ids) * self.pose_dim + (self.num_calib_params() if include_calibration else 0)
        out = np.zeros((m, m))
        o = PcgOptions(float(rel_tolerance), int(max_iterations), int(check_every), int(coarse_aggregate))
        self._chk(self.L.ba_hip_get_joint_marginals_pcg(self.h, len(ids), _p(ids, u32p), int(bool(include_calibration)),
                                                        C.byref(o), _p(out, dp)))
        return out

    def pcg_panel_stats(self):
        st = PcgPanelStats()
        self._chk(self.L.ba_hip_get_pcg_panel_stats(self.h, C.byref(st)))
        return _pcg_stats_dict(st)

    def pcg_panel_columns(self, m):
        """The per-column record of the last panel solve: dict of (m,) arrays."""
        it, cv, bd = (np.zeros(int(m), dtype=np.uint32) for _ in range(3))
        rel = np.zeros(int(m))
        self._chk(self.L.ba_hip_get_pcg_panel_columns(self.h, int(m), _p(it, u32p), _p(cv, u32p), _p(bd, u32p), _p(rel, dp)))
        return dict(iterations=it, converged=cv, breakdown=bd, rel_residual_true=rel)

    def pcg_panel_solve(self, a_lower, B, block, rel_tolerance, max_iterations=0, check_every=0, coarse_aggregate=0):
        """Stand-alone panel PCG on an SPD system given by its lower triangle: (X, rc, stats dict); B is (n, m)."""
        a, B = _d(a_lower), _d(B)
        if B.ndim == 1:
            B = B[:, None]
        B = np.ascontiguousarray(B)
        X = np.zeros_like(B)
        o = PcgOptions(float(rel_tolerance), int(max_iterations), int(check_every), int(coarse_aggregate))
        st = PcgPanelStats()
        rc = self._chk(self.L.ba_hip_pcg_panel_solve(self.h, B.shape[0], _p(a, dp), B.shape[1], _p(B, dp), int(block),
                                                     C.byref(o), _p(X, dp), C.byref(st)), positive_ok=True)
        return X, rc, _pcg_stats_dict(st)

    def dense_solve(self, a_lower, b):
        a, b = _d(a_lower), _d(b)
        x = np.empty(b.shape[0])
        rc = self._chk(self.L.ba_hip_dense_solve(self.h, b.shape[0], _p(a, dp), _p(b, dp), _p(x, dp)),
                       positive_ok=True)
        return x, rc

    def tile_solve(self, a_lower, b, tile_map=None, keep_factor=False):
        """The direct tile-sparse L D L^T solve on a symmetric system given by its lower triangle, with the lower
        64x64-tile pattern `tile_map` (nt x nt; None: the pattern of the nonzeros): (x, rc, nzL), and with
        keep_factor (x, rc, nzL, storage (64 nt)^2, linvT (nt, 64, 64), dsgn (64 nt)) — the kept factor."""
        a, b = _d(a_lower), _d(b)
        n = b.shape[0]
        nt = max((n + 63) // 64, 1)
        tm = None
        if tile_map is not None:
            tm = np.ascontiguousarray(tile_map, dtype=np.uint8)
            if tm.shape != (nt, nt):
                raise ValueError("tile_map must be %d x %d" % (nt, nt))
        x = np.zeros(n)
        nzl = np.zeros((nt, nt), dtype=np.uint8)
        st = np.zeros((64 * nt, 64 * nt)) if keep_factor else None
        li = np.zeros((nt, 64, 64)) if keep_factor else None
        sg = np.zeros(64 * nt) if keep_factor else None
        rc = self._chk(self.L.ba_hip_tile_solve(self.h, n, _p(a, dp), _p(b, dp), _p(tm, u8p), _p(x, dp), _p(nzl, u8p),
                                                _p(st, dp), _p(li, dp), _p(sg, dp)), positive_ok=True)
        return (x, rc, nzl, st, li, sg) if keep_factor else (x, rc, nzl)

    def tile_factor_solve(self, a_lower, B, tile_map=None):
        """The factorisation of tile_solve on (a_lower, tile_map), then X = A^-1 B (n x m) by the substitution of
        factor_solve on the factor it leaves: (X, rc)."""
        a, B = _d(a_lower), _d(B)
        n = a.shape[0]
        nt = max((n + 63) // 64, 1)
        tm = None
        if tile_map is not None:
            tm = np.ascontiguousarray(tile_map, dtype=np.uint8)
            if tm.shape != (nt, nt):
                raise ValueError("tile_map must be %d x %d" % (nt, nt))
        if B.ndim != 2 or B.shape[0] != n:
            raise ValueError("B must be %d x m" % n)
        X = np.zeros_like(B)
        rc = self._chk(self.L.ba_hip_tile_factor_solve(self.h, n, _p(a, dp), _p(tm, u8p), B.shape[1], _p(B, dp), _p(X, dp)),
                       positive_ok=True)
        return X, rc

    def select_kth(self, values, k):
        v = _d(values)
        out = C.c_double()
        self._chk(self.L.ba_hip_select_kth(self.h, v.shape[0], _p(v, dp), int(k), C.byref(out)))
        return out.value
