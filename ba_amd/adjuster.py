"""Python view of the C++ host class ba::BundleAdjuster<> (include/ba/BundleAdjuster.h)
through its flat C wrapper (include/ba_capi.h, ba_amd/lib/libba_capi.so).

Method names follow the reference API (/root/reference/include/ba/BundleAdjuster.h:
177-631) so parity tests can feed the same calls to this class and to the oracle.
Everything below runs on the MI355X engine; importing works without a GPU, Solve()
does not (the result is SolverError and an error line — there is no CPU fallback).
"""
import ctypes as C
import os

import numpy as np

from . import hipapi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libba_capi.so")

dp = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)

RESULT_NAMES = ["Success", "ErrorIncreased", "ErrorChangeBelowThreshold",
                "ParamChangeBelowThreshold", "FactorizationError", "SolverError"]


class BaOptions(C.Structure):
    _fields_ = [("trust_region_size", C.c_double),
                ("gyro_sigma", C.c_double), ("accel_sigma", C.c_double),
                ("gyro_bias_sigma", C.c_double), ("accel_bias_sigma", C.c_double),
                ("projection_outlier_threshold", C.c_double),
                ("error_change_threshold", C.c_double), ("param_change_threshold", C.c_double),
                ("dogleg_max_inner_iterations", C.c_uint32),
                ("apply_results", C.c_int32), ("use_dogleg", C.c_int32),
                ("use_triangular_matrices", C.c_int32), ("use_sparse_solver", C.c_int32),
                ("regularize_biases_in_batch", C.c_int32),
                ("enable_auto_regularization", C.c_int32),
                ("use_robust_norm_for_proj_residuals", C.c_int32),
                ("use_robust_norm_for_inertial_residuals", C.c_int32),
                ("write_reduced_camera_matrix", C.c_int32),
                ("device", C.c_int32), ("factorization_pivot_tolerance", C.c_double),
                ("calculate_calibration_marginals", C.c_int32), ("pose_ordering", C.c_int32),
                ("reduced_solver", C.c_int32), ("pcg_max_iterations", C.c_uint32), ("pcg_tolerance", C.c_double),
                ("pcg_coarse_aggregate", C.c_uint32), ("reserved0", C.c_uint32)]


class BaSummary(C.Structure):
    _fields_ = [("num_proj_residuals", C.c_uint32), ("num_inertial_residuals", C.c_uint32),
                ("num_cond_proj_residuals", C.c_uint32), ("num_cond_inertial_residuals", C.c_uint32),
                ("proj_error", C.c_double), ("inertial_error", C.c_double),
                ("unary_error", C.c_double), ("binary_error", C.c_double),
                ("delta_norm", C.c_double), ("pre_solve_norm", C.c_double),
                ("post_solve_norm", C.c_double), ("result", C.c_int32),
                ("iterations_run", C.c_uint32), ("trust_region_size", C.c_double)]


SYMBOLS = [
    "ba_default_options", "ba_adjuster_create", "ba_adjuster_destroy", "ba_adjuster_init",
    "ba_adjuster_set_gravity", "ba_adjuster_add_camera", "ba_adjuster_add_pose",
    "ba_adjuster_add_landmark", "ba_adjuster_add_projection_residual",
    "ba_adjuster_add_unary_constraint", "ba_adjuster_add_binary_constraint",
    "ba_adjuster_add_imu_residual", "ba_adjuster_regularize_pose", "ba_adjuster_set_root_pose_id",
    "ba_adjuster_set_pose_cam_params", "ba_adjuster_set_calculate_inertial_covariance_once", "ba_adjuster_set_imu_noise",
    "ba_adjuster_add_poses", "ba_adjuster_add_landmarks", "ba_adjuster_add_projection_residuals",
    "ba_adjuster_solve", "ba_adjuster_num_poses", "ba_adjuster_num_landmarks",
    "ba_adjuster_num_proj_residuals", "ba_adjuster_get_poses", "ba_adjuster_get_landmarks",
    "ba_adjuster_is_landmark_reliable", "ba_adjuster_landmark_outlier_ratio",
    "ba_adjuster_get_projection_residual", "ba_adjuster_get_imu_residual",
    "ba_adjuster_get_summary", "ba_adjuster_get_cond_errors", "ba_adjuster_get_timers", "ba_adjuster_engine",
    "ba_adjuster_set_allreduce", "ba_adjuster_set_communicator", "ba_adjuster_solve_is_distributed", "ba_adjuster_set_collectives", "ba_adjuster_create_calib", "ba_adjuster_get_camera_pose",
    "ba_adjuster_get_last_calib_step", "ba_adjuster_get_calibration_marginals", "ba_adjuster_get_camera_params",
    "ba_adjuster_add_camera_fov", "ba_adjuster_get_camera_fov",
    "ba_adjuster_get_pose_covariance", "ba_adjuster_get_pose_cross_covariance", "ba_adjuster_get_landmark_covariance",
    "ba_adjuster_get_projection_leverage", "ba_adjuster_get_projection_redundancy",
    "ba_adjuster_get_joint_pose_covariance",
    "ba_adjuster_get_joint_covariance", "ba_adjuster_get_pose_landmark_cross_covariance",
    "ba_adjuster_solve_with_factor", "ba_adjuster_get_weakest_modes", "ba_adjuster_get_mode_stats",
    "ba_adjuster_solve_with_pcg", "ba_adjuster_get_joint_pose_covariance_iterative", "ba_adjuster_get_pcg_panel_stats",
    "ba_adjuster_get_pose_pose_leverages", "ba_adjuster_get_pose_pose_leverage",
    "ba_adjuster_marginalize", "ba_adjuster_get_marginalization", "ba_adjuster_add_dense_prior",
    "ba_adjuster_triangulate_landmarks", "ba_adjuster_refine_poses",
    "ba_adjuster_get_pcg_stats", "ba_adjuster_get_pcg_coarse_stats",
    "ba_adjuster_set_levenberg_marquardt", "ba_adjuster_get_damping", "ba_adjuster_get_levenberg_marquardt_state",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        hipapi.lib()  # libba_capi.so links libba_hip.so; fail with the clear message first
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("ba_amd: %s is missing — run __graft_entry__.build()" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        L = _lib
        L.ba_adjuster_create.restype = C.c_void_p
        L.ba_adjuster_create_calib.restype = C.c_void_p
        L.ba_adjuster_engine.restype = C.c_void_p
        L.ba_adjuster_landmark_outlier_ratio.restype = C.c_double
        L.ba_adjuster_get_camera_fov.restype = C.c_double
        L.ba_adjuster_get_damping.restype = C.c_double
        for n in ("ba_adjuster_add_camera", "ba_adjuster_add_pose", "ba_adjuster_add_landmark",
                  "ba_adjuster_add_projection_residual", "ba_adjuster_add_unary_constraint",
                  "ba_adjuster_add_binary_constraint", "ba_adjuster_add_imu_residual",
                  "ba_adjuster_num_poses", "ba_adjuster_num_landmarks",
                  "ba_adjuster_num_proj_residuals"):
            getattr(L, n).restype = C.c_uint32
    return _lib


def default_options():
    o = BaOptions()
    lib().ba_default_options(C.byref(o))
    return o


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


class _EngineView(hipapi.Engine):
    """Debug taps (include/ba_hip.h) on the engine owned by a C++ adjuster."""

    def __init__(self, handle, lm_dim, pose_dim):  # the base constructor would create an engine
        self.L = hipapi.lib()
        self.lm_dim, self.pose_dim = lm_dim, pose_dim
        self.h = C.c_void_p(handle)
        self._cb = None

    def close(self):
        self.h = C.c_void_p()  # not owned


class BundleAdjuster:
    """ba::BundleAdjuster<double, lm_dim, pose_dim, 0, do_tvs> on the MI355X engine."""

    def __init__(self, lm_dim=1, pose_dim=6, do_tvs=False, calib_size=0):
        self.L = lib()
        self.lm_dim, self.pose_dim, self.do_tvs, self.calib_size = lm_dim, pose_dim, bool(do_tvs), int(calib_size)
        self.h = C.c_void_p(self.L.ba_adjuster_create_calib(lm_dim, pose_dim, int(calib_size), int(do_tvs)))
        if not self.h:
            raise ValueError("unsupported (lm_dim, pose_dim, calib_size, do_tvs)")
        self._cb = None

    def __del__(self):
        try:
            if self.h:
                self.L.ba_adjuster_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # -- reference API -----------------------------------------------------------
    def Init(self, options=None):
        self.options = options if options is not None else default_options()
        self.L.ba_adjuster_init(self.h, C.byref(self.options))

    def SetGravity(self, g):
        g = _d(g)
        self.L.ba_adjuster_set_gravity(self.h, _p(g, dp))

    def AddCamera(self, params, t_vs=(0, 0, 0, 0, 0, 0, 1)):
        """params (fx, fy, u0, v0): calibu::LinearCamera; (fx, fy, u0, v0, w): calibu::FovCamera."""
        p, t = _d(params), _d(t_vs)
        self._cam_fov = getattr(self, "_cam_fov", []) + [p.size == 5]
        if p.size == 5:
            return self.L.ba_adjuster_add_camera_fov(self.h, _p(p, dp), _p(t, dp))
        return self.L.ba_adjuster_add_camera(self.h, _p(p, dp), _p(t, dp))

    def AddPose(self, t_wp, is_active=True, time=-1.0, v_w=(0, 0, 0), b=(0,) * 6):
        t, v, bb = _d(t_wp), _d(v_w), _d(b)
        return self.L.ba_adjuster_add_pose(self.h, _p(t, dp), _p(v, dp), _p(bb, dp), int(is_active),
                                           C.c_double(time))

    def SetPoseCamParams(self, pose_cam_params):
        """Per-pose pinhole intrinsics (P x 4) + Options::use_per_pose_cam_params (reference
        BundleAdjuster.h:96, 292-323); None switches back to the rig camera."""
        if pose_cam_params is None:
            rc = self.L.ba_adjuster_set_pose_cam_params(self.h, 0, None)
        else:
            a = _d(pose_cam_params).reshape(-1, 4)
            rc = self.L.ba_adjuster_set_pose_cam_params(self.h, a.shape[0], _p(a, dp))
        if rc != 0:
            raise ValueError("SetPoseCamParams: one [fx, fy, u0, v0] per pose expected")

    def SetImuNoise(self, r6, rb6):
        """SetImuCalibration with other noise diagonals r / r_b (reference BundleAdjuster.h:566-567)."""
        a, b = _d(r6), _d(rb6)
        self.L.ba_adjuster_set_imu_noise(self.h, _p(a, dp), _p(b, dp))

    def SetCalculateInertialCovarianceOnce(self, on=True):
        """Options::calculate_inertial_covariance_once (reference BundleAdjuster.h:106)."""
        self.L.ba_adjuster_set_calculate_inertial_covariance_once(self.h, int(on))

    def SetUsePerPoseCamParams(self, on=True):
        if not on:
            self.SetPoseCamParams(None)

    def AddLandmark(self, x_w, ref_pose_id, ref_cam_id=0, is_active=True):
        x = _d(x_w)
        return self.L.ba_adjuster_add_landmark(self.h, _p(x, dp), int(ref_pose_id), int(ref_cam_id),
                                               int(is_active))

    def AddProjectionResidual(self, z, meas_pose_id, landmark_id, cam_id=0, weight=1.0):
        zz = _d(z)
        return self.L.ba_adjuster_add_projection_residual(self.h, _p(zz, dp), int(meas_pose_id),
                                                          int(landmark_id), int(cam_id),
                                                          C.c_double(weight))

    def AddUnaryConstraint(self, pose_id, t_wv, covariance, use_rotation=True):
        t, c = _d(t_wv), _d(covariance).reshape(36)
        return self.L.ba_adjuster_add_unary_constraint(self.h, int(pose_id), _p(t, dp), _p(c, dp),
                                                       int(use_rotation))

    def AddBinaryConstraint(self, p1, p2, t_12, covariance=None, weight=1.0, use_rotation=True):
        t = _d(t_12)
        c = _d(np.eye(6) if covariance is None else covariance).reshape(36)
        return self.L.ba_adjuster_add_binary_constraint(self.h, int(p1), int(p2), _p(t, dp),
                                                        _p(c, dp), C.c_double(weight),
                                                        int(use_rotation))

    def AddImuResidual(self, p1, p2, meas, weight=1.0):
        m = _d(meas).reshape(-1, 7)
        return self.L.ba_adjuster_add_imu_residual(self.h, int(p1), int(p2), _p(m, dp), m.shape[0],
                                                   C.c_double(weight))

    def RegularizePose(self, pose_id, translation, gravity, bias, rotation):
        self.L.ba_adjuster_regularize_pose(self.h, int(pose_id), int(translation), int(gravity),
                                           int(bias), int(rotation))

    def SetRootPoseId(self, i):
        self.L.ba_adjuster_set_root_pose_id(self.h, int(i))

    def Solve(self, max_iter, gn_damping=1.0, error_increase_allowed=False):
        self.L.ba_adjuster_solve(self.h, int(max_iter), C.c_double(gn_damping),
                                 int(error_increase_allowed))

    def SetLevenbergMarquardt(self, on, lambda0=1e-4):
        """Options::use_levenberg_marquardt / lm_initial_damping between Solve() calls: damped steps accepted by gain
        ratio; the damping starts again at lambda0."""
        self.L.ba_adjuster_set_levenberg_marquardt(self.h, int(bool(on)), C.c_double(lambda0))

    def damping(self):
        """the Levenberg-Marquardt damping the next iteration starts with"""
        return float(self.L.ba_adjuster_get_damping(self.h))

    def levenberg_marquardt_state(self):
        """(gain ratio of the last step judged, steps the last Solve() rolled back and re-linearised)"""
        rho, rej = C.c_double(), C.c_uint32()
        self.L.ba_adjuster_get_levenberg_marquardt_state(self.h, C.byref(rho), C.byref(rej))
        return rho.value, int(rej.value)

    def GetNumPoses(self):
        return self.L.ba_adjuster_num_poses(self.h)

    def GetNumLandmarks(self):
        return self.L.ba_adjuster_num_landmarks(self.h)

    def GetNumProjResiduals(self):
        return self.L.ba_adjuster_num_proj_residuals(self.h)

    def IsLandmarkReliable(self, i):
        return bool(self.L.ba_adjuster_is_landmark_reliable(self.h, int(i)))

    def LandmarkOutlierRatio(self, i):
        return self.L.ba_adjuster_landmark_outlier_ratio(self.h, int(i))

    def GetProjectionResidual(self, i):
        """dict view of ba::ProjectionResidualT (reference BundleAdjuster.h:568-571)."""
        o = np.empty(11)
        self.L.ba_adjuster_get_projection_residual(self.h, int(i), _p(o, dp))
        return {"z": o[0:2].copy(), "residual": o[2:4].copy(), "weight": o[4], "orig_weight": o[5],
                "mahalanobis_distance": o[6], "x_meas_id": int(o[7]), "x_ref_id": int(o[8]),
                "landmark_id": int(o[9]), "cam_id": int(o[10])}

    def cond_errors(self):
        """(cond_proj_error, cond_inertial_error) of the SolutionSummary (reference :680-704)."""
        o = np.empty(2)
        self.L.ba_adjuster_get_cond_errors(self.h, _p(o, dp))
        return float(o[0]), float(o[1])

    def GetImuResidual(self, i):
        """dict view of ba::ImuResidualT (reference BundleAdjuster.h:563-565)."""
        o = np.empty(19)
        self.L.ba_adjuster_get_imu_residual.restype = C.c_uint32
        n = self.L.ba_adjuster_get_imu_residual(self.h, int(i), _p(o, dp))
        return {"pose1_id": int(o[0]), "pose2_id": int(o[1]), "weight": o[2], "num_measurements": int(n),
                "residual": o[4:19].copy()}

    # -- bulk adders -----------------------------------------------------------------
    def add_poses(self, t_wp, v_w=None, b=None, is_active=None, time=None):
        t = _d(t_wp).reshape(-1, 7)
        v = _d(v_w) if v_w is not None else None
        bb = _d(b) if b is not None else None
        a = np.ascontiguousarray(is_active, dtype=np.uint8) if is_active is not None else None
        tm = _d(time) if time is not None else None
        self.L.ba_adjuster_add_poses(self.h, t.shape[0], _p(t, dp), _p(v, dp), _p(bb, dp),
                                     _p(a, u8p), _p(tm, dp))

    def add_landmarks(self, x_w, ref_pose_id, ref_cam_id=None, is_active=None):
        x = _d(x_w).reshape(-1, 4)
        rp = np.ascontiguousarray(ref_pose_id, dtype=np.uint32)
        rc = np.ascontiguousarray(ref_cam_id, dtype=np.uint32) if ref_cam_id is not None else None
        a = np.ascontiguousarray(is_active, dtype=np.uint8) if is_active is not None else None
        self.L.ba_adjuster_add_landmarks(self.h, x.shape[0], _p(x, dp), _p(rp, u32p), _p(rc, u32p),
                                         _p(a, u8p))

    def add_projection_residuals(self, z, meas_pose_id, landmark_id, cam_id=None, weight=None):
        zz = _d(z).reshape(-1, 2)
        mp = np.ascontiguousarray(meas_pose_id, dtype=np.uint32)
        li = np.ascontiguousarray(landmark_id, dtype=np.uint32)
        ci = np.ascontiguousarray(cam_id, dtype=np.uint32) if cam_id is not None else None
        w = _d(weight) if weight is not None else None
        ids = np.empty(zz.shape[0], dtype=np.uint32)
        self.L.ba_adjuster_add_projection_residuals(self.h, zz.shape[0], _p(zz, dp), _p(mp, u32p),
                                                    _p(li, u32p), _p(ci, u32p), _p(w, dp),
                                                    _p(ids, u32p))
        return ids

    # -- results -------------------------------------------------------------------------
    def poses(self):
        n = self.GetNumPoses()
        t, v, b = np.empty((n, 7)), np.empty((n, 3)), np.empty((n, 6))
        self.L.ba_adjuster_get_poses(self.h, _p(t, dp), _p(v, dp), _p(b, dp))
        return t, v, b

    def landmarks(self):
        x = np.empty((self.GetNumLandmarks(), 4))
        self.L.ba_adjuster_get_landmarks(self.h, _p(x, dp))
        return x

    def summary(self):
        s = BaSummary()
        self.L.ba_adjuster_get_summary(self.h, C.byref(s))
        return s

    def timers(self):
        t = hipapi.Timers()
        self.L.ba_adjuster_get_timers(self.h, C.byref(t))
        return {n: getattr(t, n) for n, _ in hipapi.Timers._fields_}

    # -- engine taps (valid after a Solve) -------------------------------------------------
    def engine(self):
        h = self.L.ba_adjuster_engine(self.h)
        if not h:
            raise hipapi.HipError("the adjuster has no engine yet (Solve() not run or no GPU)")
        return _EngineView(h, self.lm_dim, self.pose_dim)

    def S(self):
        return self.engine().get_S()

    def rhs(self):
        return self.engine().get_rhs()[0]

    def rhs_p(self):
        return self.engine().get_rhs()[1]

    def rhs_l(self):
        return self.engine().get_rhs()[2]

    def delta_p(self):
        e = self.engine()
        return e.get_step()[0][:e.num_pose_params()]

    def delta_k(self):
        e = self.engine()
        return e.get_step()[0][e.num_pose_params():]

    def rhs_k(self):
        e = self.engine()
        return e.get_rhs()[1][e.num_pose_params():]

    def num_pose_params(self):
        return self.engine().num_pose_params()

    def proj_tvs_jacobians(self):
        return self.engine().get_calib_jacobians(self.GetNumProjResiduals())

    def calibration_marginals(self):
        """SolutionSummary::calibration_marginals (empty without the option / without do_tvs)."""
        c = np.zeros(36)
        self.L.ba_adjuster_get_calibration_marginals.restype = C.c_uint32
        k = self.L.ba_adjuster_get_calibration_marginals(self.h, c.ctypes.data_as(C.POINTER(C.c_double)))
        return c[:k * k].reshape(k, k)

    def Marginalize(self, pose_ids, lm_ids=()):
        """ba::BundleAdjuster::Marginalize after a Solve(): a dict with pose_ids (the blanket), x0 (|B| x 16), H, b,
        c and dropped_projection.  Raises RuntimeError when refused."""
        m = np.ascontiguousarray(pose_ids, dtype=np.uint32)
        l = np.ascontiguousarray(lm_ids, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        nb = C.c_uint32(0)
        rc = self.L.ba_adjuster_marginalize(self.h, len(m), m.ctypes.data_as(u32p) if len(m) else None, len(l),
                                            l.ctypes.data_as(u32p) if len(l) else None, C.byref(nb))
        if rc != 0:
            raise RuntimeError("Marginalize refused (see stderr)")
        n, D = nb.value, self.pose_dim
        ids = np.zeros(max(n, 1), dtype=np.uint32)
        x0 = np.zeros((max(n, 1), 16))
        H = np.zeros((max(n * D, 1), max(n * D, 1)))
        b = np.zeros(max(n * D, 1))
        c = C.c_double(0.0)
        dr = C.c_uint32(0)
        dp = C.POINTER(C.c_double)
        self.L.ba_adjuster_get_marginalization(self.h, ids.ctypes.data_as(u32p), x0.ctypes.data_as(dp),
                                               H.ctypes.data_as(dp), b.ctypes.data_as(dp), C.byref(c), C.byref(dr))
        return {"pose_ids": ids[:n], "x0": x0[:n], "H": H[:n * D, :n * D], "b": b[:n * D], "c": c.value,
                "dropped_projection": dr.value}

    def TriangulateLandmarks(self, ids=None, **options):
        """ba::BundleAdjuster::TriangulateLandmarks, before or between Solve() calls: ids None = every landmark; options:
        the fields of hipapi.TriangulationOptions.  Returns (ok, results n x 8); ok False when refused (see stderr)."""
        o = hipapi.TriangulationOptions(**options)
        u32p = C.POINTER(C.c_uint32)
        if ids is None:
            n, idp = self.GetNumLandmarks(), None
        else:
            ida = np.ascontiguousarray(ids, dtype=np.uint32)
            n, idp = len(ida), ida.ctypes.data_as(u32p)
        res = np.zeros((max(n, 1), 8))
        rc = self.L.ba_adjuster_triangulate_landmarks(self.h, n, idp, C.byref(o), res.ctypes.data_as(C.POINTER(C.c_double)))
        return rc == 0, res[:n]

    def RefinePoses(self, ids=None, **options):
        """ba::BundleAdjuster::RefinePoses, before or between Solve() calls: ids None = every pose; options: the fields of
        hipapi.PoseRefinementOptions.  Returns (ok, results n x 8, t_wp n x 7, info n x 6 x 6); ok False when refused (see
        stderr)."""
        o = hipapi.PoseRefinementOptions(**options)
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        if ids is None:
            n, idp = self.GetNumPoses(), None
        else:
            ida = np.ascontiguousarray(ids, dtype=np.uint32)
            n, idp = len(ida), ida.ctypes.data_as(u32p)
        res, t7, info = np.zeros((max(n, 1), 8)), np.zeros((max(n, 1), 7)), np.zeros((max(n, 1), 6, 6))
        rc = self.L.ba_adjuster_refine_poses(self.h, n, idp, C.byref(o), res.ctypes.data_as(dp), t7.ctypes.data_as(dp),
                                             info.ctypes.data_as(dp))
        return rc == 0, res[:n], t7[:n], info[:n]

    def engine_landmarks(self):
        """ba_hip_get_landmarks of the adjuster's engine"""
        return self.engine().get_landmarks(self.GetNumLandmarks())

    def AddDensePrior(self, pose_ids, prior):
        """ba::BundleAdjuster::AddDensePrior: pose_ids of this problem, in the order of prior["pose_ids"]."""
        ids = np.ascontiguousarray(pose_ids, dtype=np.uint32)
        x0 = np.ascontiguousarray(prior["x0"], dtype=np.float64)
        H = np.ascontiguousarray(prior["H"], dtype=np.float64)
        b = np.ascontiguousarray(prior["b"], dtype=np.float64)
        k, D = len(ids), self.pose_dim
        if (k == 0 or len(prior["pose_ids"]) != k or x0.size != 16 * k or H.size != (k * D) ** 2 or
                b.size != k * D):
            raise RuntimeError("AddDensePrior: the sizes of the prior do not match its %d poses" % k)
        dp = C.POINTER(C.c_double)
        self.L.ba_adjuster_add_dense_prior.restype = C.c_uint32
        r = self.L.ba_adjuster_add_dense_prior(self.h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               x0.ctypes.data_as(dp), H.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                               C.c_double(float(prior["c"])))
        if r == 0xFFFFFFFF:
            raise RuntimeError("AddDensePrior refused (see stderr)")
        return r

    def pose_covariance(self, pose_id, other=None):
        """GetPoseCovariance (or GetPoseCrossCovariance with `other`): PoseSize x PoseSize; raises when
        unavailable."""
        D = self.pose_dim
        c = np.zeros(D * D)
        cp = c.ctypes.data_as(C.POINTER(C.c_double))
        if other is None:
            self.L.ba_adjuster_get_pose_covariance.restype = C.c_uint32
            k = self.L.ba_adjuster_get_pose_covariance(self.h, int(pose_id), cp)
        else:
            self.L.ba_adjuster_get_pose_cross_covariance.restype = C.c_uint32
            k = self.L.ba_adjuster_get_pose_cross_covariance(self.h, int(pose_id), int(other), cp)
        if k != D:
            raise RuntimeError("pose covariance of pose %d unavailable (see stderr)" % pose_id)
        return c.reshape(D, D)

    def GetJointPoseCovariance(self, ids, include_calibration=False):
        """GetJointPoseCovariance: the (M, M) joint covariance of the poses `ids` in the given order, M =
        len(ids) * PoseSize (+ the calibration rows last); raises when unavailable."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32).ravel()
        k = self.L.ba_hip_num_calib_params(self.engine().h) if include_calibration else 0
        m = len(ids) * self.pose_dim + k
        c = np.zeros((m, m))
        self.L.ba_adjuster_get_joint_pose_covariance.restype = C.c_uint32
        got = self.L.ba_adjuster_get_joint_pose_covariance(self.h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                           int(bool(include_calibration)),
                                                           c.ctypes.data_as(C.POINTER(C.c_double)))
        if got != m or m == 0:
            raise RuntimeError("joint pose covariance unavailable (see stderr)")
        return c

    def GetJointCovariance(self, pose_ids, landmark_ids, include_calibration=False):
        """GetJointCovariance: the (M, M) block of the inverse of the full system over the poses, the calibration rows
        (when asked for) and the landmarks, columns in that order; raises when unavailable."""
        pose_ids = np.ascontiguousarray(np.atleast_1d(pose_ids), dtype=np.uint32).ravel()
        landmark_ids = np.ascontiguousarray(np.atleast_1d(landmark_ids), dtype=np.uint32).ravel()
        k = self.L.ba_hip_num_calib_params(self.engine().h) if include_calibration else 0
        m = len(pose_ids) * self.pose_dim + k + len(landmark_ids) * self.lm_dim
        c = np.zeros((m, m))
        u32p = C.POINTER(C.c_uint32)
        self.L.ba_adjuster_get_joint_covariance.restype = C.c_uint32
        got = self.L.ba_adjuster_get_joint_covariance(self.h, len(pose_ids), pose_ids.ctypes.data_as(u32p),
                                                      int(bool(include_calibration)), len(landmark_ids),
                                                      landmark_ids.ctypes.data_as(u32p),
                                                      c.ctypes.data_as(C.POINTER(C.c_double)))
        if got != m or m == 0:
            raise RuntimeError("joint covariance unavailable (see stderr)")
        return c

    def _reduced_rows(self):
        eh = self.engine().h
        return int(self.L.ba_hip_num_pose_params(eh)) + int(self.L.ba_hip_num_calib_params(eh))

    def SolveWithFactor(self, B):
        """SolveWithFactor: X = S^-1 B with the factor of the last Solve(); B is (n, m), rows as delta_p() then the
        calibration rows; raises when unavailable."""
        B = np.ascontiguousarray(B, dtype=np.float64)
        n = self._reduced_rows()
        if B.ndim != 2 or B.shape[0] != n:
            raise RuntimeError("SolveWithFactor: B must be (%d, m)" % n)
        X = np.zeros_like(B)
        dp = C.POINTER(C.c_double)
        if self.L.ba_adjuster_solve_with_factor(self.h, n, B.shape[1], B.ctypes.data_as(dp), X.ctypes.data_as(dp)):
            raise RuntimeError("solve with the factor unavailable (see stderr)")
        return X

    def SolveWithPcg(self, B, tol=0.0):
        """SolveWithPcg: X = S^-1 B without a factor, after a Solve() with reduced_solver = Pcg; B as in
        SolveWithFactor, tol the relative residual per column (0: Options.pcg_tolerance); raises when unavailable."""
        B = np.ascontiguousarray(B, dtype=np.float64)
        n = self._reduced_rows()
        if B.ndim != 2 or B.shape[0] != n:
            raise RuntimeError("SolveWithPcg: B must be (%d, m)" % n)
        X = np.zeros_like(B)
        dp = C.POINTER(C.c_double)
        if self.L.ba_adjuster_solve_with_pcg(self.h, n, B.shape[1], B.ctypes.data_as(dp), C.c_double(tol), X.ctypes.data_as(dp)):
            raise RuntimeError("solve with the panel PCG unavailable (see stderr)")
        return X

    def GetJointPoseCovarianceIterative(self, ids, tol=0.0, include_calibration=False):
        """GetJointPoseCovarianceIterative: GetJointPoseCovariance after a Solve() with reduced_solver = Pcg."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32).ravel()
        k = self.L.ba_hip_num_calib_params(self.engine().h) if include_calibration else 0
        m = len(ids) * self.pose_dim + k
        c = np.zeros((m, m))
        self.L.ba_adjuster_get_joint_pose_covariance_iterative.restype = C.c_uint32
        got = self.L.ba_adjuster_get_joint_pose_covariance_iterative(
            self.h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_uint32)), int(bool(include_calibration)), C.c_double(tol),
            c.ctypes.data_as(C.POINTER(C.c_double)))
        if got != m or m == 0:
            raise RuntimeError("iterative joint pose covariance unavailable (see stderr)")
        return c

    def GetPcgPanelStats(self):
        st = hipapi.PcgPanelStats()
        if self.L.ba_adjuster_get_pcg_panel_stats(self.h, C.byref(st)):
            return None
        return {k: getattr(st, k) for k, _ in hipapi.PcgPanelStats._fields_}

    def GetWeakestModes(self, k):
        """GetWeakestModes: (eigenvalues (k,), modes (k, n)) of smallest magnitude of the reduced system of the last
        Solve(), each mode a unit vector over the rows of SolveWithFactor; raises when unavailable."""
        n = self._reduced_rows()
        lam, modes = np.zeros(int(k)), np.zeros((int(k), n))
        dp = C.POINTER(C.c_double)
        if self.L.ba_adjuster_get_weakest_modes(self.h, int(k), n, lam.ctypes.data_as(dp), modes.ctypes.data_as(dp)):
            raise RuntimeError("weakest modes unavailable (see stderr)")
        return lam, modes

    def GetModeStats(self):
        st = hipapi.ModeStats()
        if self.L.ba_adjuster_get_mode_stats(self.h, C.byref(st)):
            raise RuntimeError("mode statistics unavailable")
        return {k: getattr(st, k) for k, _ in hipapi.ModeStats._fields_ if k != "reserved"}

    def GetPoseLandmarkCrossCovariance(self, pose_id, landmark_id):
        """GetPoseLandmarkCrossCovariance: the (PoseSize, LmSize) block Cov(pose, landmark); raises when unavailable."""
        c = np.zeros((self.pose_dim, self.lm_dim))
        if self.L.ba_adjuster_get_pose_landmark_cross_covariance(self.h, int(pose_id), int(landmark_id),
                                                                 c.ctypes.data_as(C.POINTER(C.c_double))):
            raise RuntimeError("pose-landmark cross covariance unavailable (see stderr)")
        return c

    def landmark_covariance(self, landmark_id):
        """GetLandmarkCovariance: LmSize x LmSize; raises when unavailable."""
        m = self.lm_dim
        c = np.zeros(m * m)
        self.L.ba_adjuster_get_landmark_covariance.restype = C.c_uint32
        k = self.L.ba_adjuster_get_landmark_covariance(self.h, int(landmark_id), c.ctypes.data_as(C.POINTER(C.c_double)))
        if k != m:
            raise RuntimeError("landmark covariance of landmark %d unavailable (see stderr)" % landmark_id)
        return c.reshape(m, m)

    def projection_leverage(self, residual_id):
        """GetProjectionLeverage: the 2 x 2 hat block of an accepted projection residual; raises when unavailable."""
        h = np.zeros(4)
        self.L.ba_adjuster_get_projection_leverage.restype = C.c_uint32
        k = self.L.ba_adjuster_get_projection_leverage(self.h, C.c_uint32(int(residual_id) & 0xFFFFFFFF),
                                                       h.ctypes.data_as(C.POINTER(C.c_double)))
        if k != 2:
            raise RuntimeError("leverage of projection residual %d unavailable (see stderr)" % residual_id)
        return h.reshape(2, 2)

    def projection_redundancy(self, residual_id):
        """GetProjectionRedundancy: 2 - trace of the hat block; raises when unavailable."""
        r = C.c_double()
        if self.L.ba_adjuster_get_projection_redundancy(self.h, C.c_uint32(int(residual_id) & 0xFFFFFFFF), C.byref(r)):
            raise RuntimeError("redundancy of projection residual %d unavailable (see stderr)" % residual_id)
        return r.value

    def pose_pose_leverages(self, kind, ids=None, count=None):
        """GetPosePoseLeverages: (cov, info, leverage) = ((n, 15, 15), (n, 15, 15), (n,)) of the unary / binary /
        inertial residuals `ids` (kind: hipapi.RES_UNARY / RES_BINARY / RES_IMU; ids=None: every residual of the
        kind in id order, `count` of them); raises when unavailable."""
        dp, n = C.POINTER(C.c_double), count
        if ids is not None:
            ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.uint32).ravel()
            n = len(ids)
        elif n is None:
            raise ValueError("pose_pose_leverages: ids=None needs the residual count of the kind")
        cov, info, lev = np.zeros((n, 15, 15)), np.zeros((n, 15, 15)), np.zeros(n)
        if self.L.ba_adjuster_get_pose_pose_leverages(
                self.h, int(kind), int(n), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                cov.ctypes.data_as(dp), info.ctypes.data_as(dp), lev.ctypes.data_as(dp)):
            raise RuntimeError("pose-pose leverages of kind %d unavailable (see stderr)" % kind)
        return cov, info, lev

    def _pose_pose_leverage(self, kind, residual_id):
        r = C.c_double()
        if self.L.ba_adjuster_get_pose_pose_leverage(self.h, int(kind), C.c_uint32(int(residual_id) & 0xFFFFFFFF),
                                                     C.byref(r)):
            raise RuntimeError("leverage of residual %d of kind %d unavailable (see stderr)" % (residual_id, kind))
        return r.value

    def GetUnaryLeverage(self, residual_id):
        """GetUnaryLeverage: tr(C Lambda) of a unary residual; raises when unavailable."""
        return self._pose_pose_leverage(hipapi.RES_UNARY, residual_id)

    def GetBinaryLeverage(self, residual_id):
        """GetBinaryLeverage: tr(C Lambda) of a binary residual; raises when unavailable."""
        return self._pose_pose_leverage(hipapi.RES_BINARY, residual_id)

    def GetImuLeverage(self, residual_id):
        """GetImuLeverage: tr(C Lambda) of an inertial residual; raises when unavailable."""
        return self._pose_pose_leverage(hipapi.RES_IMU, residual_id)

    def camera_params(self, cam_id=0):
        """rig()->cameras_[cam_id]->GetParams()"""
        p = np.empty(4)
        self.L.ba_adjuster_get_camera_params(self.h, int(cam_id), p.ctypes.data_as(C.POINTER(C.c_double)))
        if getattr(self, "_cam_fov", [])[cam_id:cam_id + 1] == [True]:
            p = np.append(p, self.L.ba_adjuster_get_camera_fov(self.h, int(cam_id)))
        return p

    def proj_calib_jacobians(self):
        """sqrt(w) dz_dk per residual id in the j_kpr_ layout, 2 x kCalibDim."""
        e = self.engine()
        return e.get_calib_jacobians(self.GetNumProjResiduals())[:, :, :e.num_calib_params()]

    def camera_pose(self, cam_id=0):
        """rig()->cameras_[cam_id]->Pose()"""
        t = np.empty(7)
        self.L.ba_adjuster_get_camera_pose(self.h, int(cam_id), t.ctypes.data_as(C.POINTER(C.c_double)))
        return t

    def delta_l(self):
        return self.engine().get_step()[1]

    def proj_weights(self):
        return self.engine().get_proj_weights(self.GetNumProjResiduals())

    def set_allreduce(self, fn, rank, nranks):
        """fn(dev_ptr:int, count:int, dtype:int) -> int; kept alive by this object."""
        if fn is None:
            self._cb = None
            self.L.ba_adjuster_set_allreduce(self.h, None, None, 0, 1)
            return
        self._cb = hipapi.ALLREDUCE_FN(lambda ctx, ptr, count, dtype: int(fn(ptr, count, dtype)))
        self.L.ba_adjuster_set_allreduce(self.h, self._cb, None, int(rank), int(nranks))

    def set_communicator(self, unique_id, rank, nranks, distributed_solve=True):
        """ba::BundleAdjuster::SetCommunicator: the engine's own RCCL communicator (unique_id = 128 bytes from
        hipapi.Engine.comm_unique_id() on rank 0); None clears it.  The next Solve() joins (collective)."""
        if unique_id is None:
            self.L.ba_adjuster_set_communicator(self.h, None, 0, 1, 0)
            return
        self.L.ba_adjuster_set_communicator(self.h, C.c_char_p(unique_id), int(rank), int(nranks), 1 if distributed_solve else 0)

    def GetPcgCoarseStats(self):
        """ba::BundleAdjuster::GetPcgCoarseStats: the coarse space of the last reduced solve as a dict when
        Options::pcg_coarse_aggregate was in force, None otherwise."""
        st = hipapi.PcgCoarseStats()
        if not self.L.ba_adjuster_get_pcg_coarse_stats(self.h, C.byref(st)):
            return None
        return hipapi._pcg_stats_dict(st)

    def GetPcgStats(self):
        """ba::BundleAdjuster::GetPcgStats: the statistics of the last reduced solve as a dict when it ran the PCG
        solver (Options reduced_solver = 1), None otherwise."""
        st = hipapi.PcgStats()
        if not self.L.ba_adjuster_get_pcg_stats(self.h, C.byref(st)):
            return None
        return {k: getattr(st, k) for k, _ in hipapi.PcgStats._fields_}

    def solve_is_distributed(self):
        return bool(self.L.ba_adjuster_solve_is_distributed(self.h))

    def set_collectives(self, fn):
        """ba::BundleAdjuster::SetCollectives: fn(op, dev_ptr, count, root) -> int, on top of set_allreduce."""
        if fn is None:
            self._cb2 = None
            self.L.ba_adjuster_set_collectives(self.h, None, None)
            return
        self._cb2 = hipapi.COLLECTIVE_FN(lambda ctx, op, ptr, count, root: int(fn(op, ptr, count, root)))
        self.L.ba_adjuster_set_collectives(self.h, self._cb2, None)
