"""Parity of the MI355X path with the oracle, through the C-ABI (include/ba_hip.h) and
the C++ host class (include/ba/BundleAdjuster.h via include/ba_capi.h).

Tolerances: BASELINE.json north_star asks for the pose update delta_x within 1e-6
relative of the CPU path; the kernels are FP64 and deterministic (no atomics), so the
assertions here are set 2-4 orders tighter and documented per quantity.
"""
import glob
import os

import numpy as np
import pytest

from ba_amd import adjuster, hipapi, scene
from helpers import accepted_obs, fill, gn_options, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1_*.npz")))


def hip_options(**kw):
    o = adjuster.default_options()
    o.use_dogleg = 0
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    o.write_reduced_camera_matrix = 1  # keep S readable after the in-place factorisation
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def both(po, sc, lm_dim, active=None, lm_active=None, pose_dim=6, **kw):
    o = po.OracleBundleAdjuster(lm_dim, pose_dim)
    o.Init(gn_options(po, **kw))
    h = adjuster.BundleAdjuster(lm_dim, pose_dim)
    h.Init(hip_options(**kw))
    fill(o, sc, active=active, lm_active=lm_active)
    fill(h, sc, active=active, lm_active=lm_active)
    return o, h


# ---- stand-alone kernels ---------------------------------------------------------------
def test_select_kth_is_exact():
    eng = hipapi.Engine(1, 6)
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 255, 256, 257, 1000, 65536, 65537, 100001, 1 << 20):  # <= 65536: the one-workgroup kernel
        v = rng.random(n) ** 3 * 50
        v[rng.integers(0, n, max(1, n // 10))] = 0.0  # ties and exact zeros
        for k in {0, n // 2, n - 1}:
            assert eng.select_kth(v, k) == np.sort(v)[k]
    # heavy ties: the k-th element is a repeated value
    v = np.repeat(np.array([3.0, 1.0, 2.0]), 1000)
    assert eng.select_kth(v, 1500) == 2.0


def test_dense_cholesky_solve_matches_numpy():
    eng = hipapi.Engine(1, 6)
    rng = np.random.default_rng(1)
    for n in (1, 5, 63, 64, 65, 100, 300, 1000, 2048):
        m = rng.normal(size=(n, n))
        a = m @ m.T + n * np.eye(n)
        b = rng.normal(size=n)
        x, rc = eng.dense_solve(np.tril(a), b)
        assert rc == 0
        assert rel_err(x, np.linalg.solve(a, b)) < 1e-11
    # symmetric indefinite (quasi-definite) systems factor as L D L^T like the reference's
    # un-pivoted LDLT (BundleAdjuster.cpp:752-761)
    # (2100: 33 tiles — with BA_HIP_BULK_FULL_M=16 (test_blocked_128_trailing_update_on_small_systems)
    # the negative pivots send k_update128's blocks through its generic 64-tile fallback)
    for n in (10, 130, 500, 2100):
        m = rng.normal(size=(n, n))
        a = m @ m.T + n * np.eye(n)
        a[n // 2:, n // 2:] -= 2.5 * (m @ m.T + n * np.eye(n))[n // 2:, n // 2:]
        b = rng.normal(size=n)
        x, rc = eng.dense_solve(np.tril(a), b)
        assert rc == 0
        assert rel_err(a @ x, b) < 1e-9
    # an exactly singular pivot is reported as FactorizationError (ba::FactorizationError = 4)
    a = np.zeros((10, 10))
    _, rc = eng.dense_solve(a, np.ones(10))
    assert rc == 4


# ---- one linearisation: S, rhs, weights, step -------------------------------------------
@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("variant", ["anchored", "inactive_mix", "root_masked", "full_matrix"])
def test_reduced_system_and_step(oracle_lib, lm_dim, variant):
    po = oracle_lib
    sc = scene.make_scene(30, 60, 5, lm_dim=lm_dim, seed=7)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    if variant in ("anchored", "full_matrix"):
        pa[sc.anchor_poses] = 0
    if variant == "inactive_mix":
        pa[[0, 3, 4, 17]] = 0
        la[[5, 6, 40]] = 0
    kw = dict(apply_results=0)
    if variant == "full_matrix":
        kw["use_triangular_matrices"] = 0
    o, h = both(po, sc, lm_dim, active=pa, lm_active=la, **kw)
    o.Solve(1)
    h.Solve(1)
    # bit-level agreement is not expected (different summation order); FP64 rounding only
    assert rel_err(h.S(), o.S()) < 1e-12
    assert rel_err(h.rhs(), o.rhs()) < 1e-11
    assert rel_err(h.rhs_p(), o.rhs_p()) < 1e-11
    assert rel_err(h.rhs_l(), o.rhs_l()) < 1e-11
    assert rel_err(h.proj_weights(), o.proj_weights()) < 1e-12
    if variant != "root_masked":
        # all-active monocular problems keep a free scale gauge: S is singular there and
        # the step is solver-dependent (tests/test_oracle_dense.py); compare the rest
        assert rel_err(h.delta_p(), o.delta_p()) < 1e-8   # north_star: 1e-6
        assert rel_err(h.delta_l(), o.delta_l()) < 1e-8


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_fixtures(path):
    g = np.load(path)
    h = adjuster.BundleAdjuster(int(g["lm_dim"]), 6)
    h.Init(hip_options(use_dogleg=int(g["use_dogleg"])))
    h.AddCamera(g["cam_params"])
    h.add_poses(g["poses"], is_active=g["pose_active"])
    h.add_landmarks(g["landmarks"], g["lm_ref_pose"])
    h.add_projection_residuals(g["obs_z"], g["obs_pose"], g["obs_lm"])
    h.Solve(1)
    assert rel_err(h.S(), g["S_it0"]) < 1e-12
    assert rel_err(h.rhs(), g["rhs_it0"]) < 1e-11
    assert rel_err(h.delta_p(), g["delta_p_it0"]) < 1e-8
    assert rel_err(h.delta_l(), g["delta_l_it0"]) < 1e-8
    assert abs(h.summary().proj_error - float(g["proj_error_it0"])) < 1e-9 * float(g["proj_error_it0"])
    for _ in range(int(g["iters"]) - 1):
        h.Solve(1)
    t, _, _ = h.poses()
    assert rel_err(t, g["poses_final"]) < 1e-8
    assert rel_err(h.landmarks(), g["landmarks_final"]) < 1e-8


# ---- several iterations: state, errors, accept/reject ------------------------------------
@pytest.mark.parametrize("lm_dim", [1, 3])
def test_gauss_newton_iterations_track_oracle(oracle_lib, lm_dim):
    po = oracle_lib
    sc = scene.make_scene(50, 200, 10, lm_dim=lm_dim, seed=1)  # BASELINE.json configs[0]
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, lm_dim, active=pa)
    for it in range(5):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        assert abs(so.proj_error - sh.proj_error) < 1e-8 * so.proj_error
        assert abs(so.delta_norm - sh.delta_norm) < 1e-7 * so.delta_norm
    to, _, _ = o.poses()
    th, _, _ = h.poses()
    assert rel_err(th, to) < 1e-8
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-8
    for l in range(sc.num_landmarks):
        assert o.IsLandmarkReliable(l) == h.IsLandmarkReliable(l)
        assert o.LandmarkOutlierRatio(l) == h.LandmarkOutlierRatio(l)


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("trust_region", [-1.0, 0.05, 1e3])
def test_dogleg_matches_oracle(oracle_lib, lm_dim, trust_region):
    """Dogleg branch (BundleAdjuster.cpp:850-1083): auto trust region, a tiny one (scaled
    steepest descent / blended steps, inner-loop rejections) and a huge one (pure GN)."""
    po = oracle_lib
    sc = scene.make_scene(40, 120, 6, lm_dim=lm_dim, seed=21)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, lm_dim, active=pa, use_dogleg=1, trust_region_size=trust_region)
    for it in range(4):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        assert abs(so.trust_region_size - sh.trust_region_size) <= 1e-7 * abs(so.trust_region_size)
        assert abs(so.pre_solve_norm - sh.pre_solve_norm) < 1e-8 * so.pre_solve_norm
        assert abs(so.post_solve_norm - sh.post_solve_norm) < 1e-8 * so.post_solve_norm
        assert abs(so.delta_norm - sh.delta_norm) < 1e-6 * max(so.delta_norm, 1e-12)
    to, _, _ = o.poses()
    th, _, _ = h.poses()
    assert rel_err(th, to) < 1e-8
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-8


def test_multi_iteration_solve_equals_repeated_single(oracle_lib):
    po = oracle_lib
    sc = scene.make_scene(40, 120, 6, lm_dim=1, seed=3)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, 1, active=pa)
    o.Solve(4)
    h.Solve(4)
    assert o.summary().iterations_run == h.summary().iterations_run
    to, _, _ = o.poses()
    th, _, _ = h.poses()
    assert rel_err(th, to) < 1e-8


def test_error_increase_is_rolled_back(oracle_lib):
    """A damped-up step (gn_damping = 40) overshoots: both paths must reject it, restore
    the state and report ErrorIncreased (BundleAdjuster.cpp:1139-1152)."""
    po = oracle_lib
    sc = scene.make_scene(30, 60, 5, lm_dim=1, seed=9)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, 1, active=pa)
    o.Solve(1, 40.0)
    h.Solve(1, 40.0)
    assert adjuster.RESULT_NAMES[h.summary().result] == "ErrorIncreased"
    assert o.summary().result == h.summary().result
    th, _, _ = h.poses()
    assert rel_err(th, sc.poses) < 1e-12  # state restored exactly (snapshot buffer)


# ---- pose-pose residuals: unary, binary, IMU ------------------------------------------------
def _state_close(o, h, tol=1e-8):
    to, vo, bo = o.poses()
    th, vh, bh = h.poses()
    assert rel_err(th, to) < tol
    assert np.abs(vh - vo).max() <= tol * max(1.0, np.abs(vo).max())
    assert np.abs(bh - bo).max() <= tol * max(1.0, np.abs(bo).max())


@pytest.mark.parametrize("use_dogleg", [0, 1])
def test_pose_graph_unary_binary(oracle_lib, use_dogleg):
    """LmSize = 0 pose graph (the shape of applications/unary_binary_imu_test): GPS-like
    unary priors with and without rotation, odometry-like binary constraints with full
    covariances and weights."""
    po = oracle_lib
    rng = np.random.default_rng(41)
    gt, _ = scene.trajectory(30)
    init = gt.copy()
    init[:, :3] += rng.normal(0, 0.05, (30, 3))
    for i in range(30):
        init[i] = po.exp_decoupled(init[i], np.concatenate([np.zeros(3), rng.normal(0, 0.02, 3)]))
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, use_dogleg=use_dogleg)),
                      (adjuster.BundleAdjuster, hip_options(use_dogleg=use_dogleg))):
        b = cls(0, 6)
        b.Init(opts)
        b.add_poses(init)
        r2 = np.random.default_rng(42)
        for i in range(0, 30, 3):
            m = r2.normal(size=(6, 6))
            cov = 1e-3 * (m @ m.T + 6 * np.eye(6))
            prior = po.exp_decoupled(gt[i], r2.normal(0, 0.01, 6))
            b.AddUnaryConstraint(i, prior, cov, bool(i % 2 == 0))
        for i in range(29):
            m = r2.normal(size=(6, 6))
            cov = 1e-4 * (m @ m.T + 6 * np.eye(6))
            t12 = po.se3_mul(po.se3_inv(gt[i]), gt[i + 1])
            t12 = po.exp_decoupled(t12, r2.normal(0, 0.003, 6))
            b.AddBinaryConstraint(i, i + 1, t12, cov, float(r2.uniform(0.5, 2.0)), bool(i % 5 != 0))
        b.AddBinaryConstraint(0, 29, po.se3_mul(po.se3_inv(gt[0]), gt[29]))  # loop closure, identity cov
        objs.append(b)
    o, h = objs
    for it in range(4):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        if so.delta_norm < 1e-9:
            # converged: the accept test post <= pre is decided by the last bit of two
            # equal sums, which no two implementations share
            break
        assert so.result == sh.result
        if it == 0:
            assert rel_err(h.S(), o.S()) < 1e-11
            assert rel_err(h.rhs(), o.rhs()) < 1e-10
        assert abs(so.unary_error - sh.unary_error) <= 1e-8 * max(so.unary_error, 1e-12)
        assert abs(so.binary_error - sh.binary_error) <= 1e-8 * max(so.binary_error, 1e-12)
        assert abs(so.delta_norm - sh.delta_norm) <= 1e-6 * max(so.delta_norm, 1e-12)
    _state_close(o, h)


@pytest.mark.parametrize("lm_dim,pose_dim", [(1, 15), (3, 15), (1, 9), (0, 15), (0, 9)])
@pytest.mark.parametrize("use_dogleg", [0, 1])
def test_visual_inertial(oracle_lib, lm_dim, pose_dim, use_dogleg):
    """BASELINE.json configs[2] in miniature: reprojection + IMU pre-integration residuals,
    velocities (and biases) in the state, gravity-axis gauge regularisation."""
    po = oracle_lib
    P = 30
    sc = scene.make_scene(P, 80 if lm_dim else 1, 5, lm_dim=max(lm_dim, 1), seed=51)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, use_dogleg=use_dogleg)),
                      (adjuster.BundleAdjuster, hip_options(use_dogleg=use_dogleg))):
        b = cls(lm_dim, pose_dim)
        b.Init(opts)
        b.SetGravity(sc.gravity)
        if lm_dim:
            fill(b, sc)
        else:
            b.add_poses(sc.poses, v_w=sc.init_vel, b=sc.init_bias, time=sc.pose_time)
            for i in range(0, P, 5):  # a single prior leaves cond(S) ~ 1e16: solver-dependent
                b.AddUnaryConstraint(i, sc.gt_poses[i], 1e-4 * np.eye(6), True)
        for i in range(P - 1):
            b.AddImuResidual(i, i + 1, sc.imu_meas[i])
        objs.append(b)
    o, h = objs
    for it in range(3):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        if it == 0:
            assert rel_err(h.S(), o.S()) < 1e-9
            assert rel_err(h.rhs(), o.rhs()) < 1e-9
        # cond(S) reaches 1e9-1e10 with velocities and biases in the state: the step agrees
        # to ~cond * eps; north_star asks for 1e-6 relative
        assert abs(so.inertial_error - sh.inertial_error) <= 1e-6 * max(so.inertial_error, 1e-12)
        assert abs(so.proj_error - sh.proj_error) <= 1e-6 * max(so.proj_error, 1e-12)
    _state_close(o, h, 1e-6)


# ---- edge cases ---------------------------------------------------------------------------
def test_weights_cameras_with_extrinsics_and_duplicate_observations(oracle_lib):
    po = oracle_lib
    rng = np.random.default_rng(4)
    sc = scene.make_scene(30, 50, 5, lm_dim=1, seed=11)
    tvs = np.concatenate([rng.normal(0, 0.05, 3), po.so3_exp(rng.normal(0, 0.1, 3))])
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    w = rng.uniform(0.5, 2.0, len(sc.obs_pose))
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, apply_results=0)),
                      (adjuster.BundleAdjuster, hip_options(apply_results=0))):
        b = cls(1, 6)
        b.Init(opts)
        b.AddCamera(sc.cam_params, tvs)
        b.add_poses(sc.poses, is_active=pa)
        b.add_landmarks(sc.landmarks, sc.lm_ref_pose)
        b.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm, weight=w)
        # the same landmark seen twice from one pose (two residuals, one incidence)
        b.add_projection_residuals(sc.obs_z[1:6] + 0.3, sc.obs_pose[1:6], sc.obs_lm[1:6])
        b.Solve(1)
        objs.append(b)
    o, h = objs
    assert rel_err(h.S(), o.S()) < 1e-12
    assert rel_err(h.rhs(), o.rhs()) < 1e-11
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-8


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("rig", ["fov", "fov_and_pinhole"])
def test_fov_camera_matches_oracle(oracle_lib, lm_dim, rig):
    """calibu::FovCamera (fx, fy, u0, v0, w — the camera of the reference's CalibSize = 5 instantiations)
    in the ordinary adjuster: residuals, reduced system and step of the first iteration, then three
    iterations of the whole solver against the oracle.  fov_and_pinhole: a rig of a FovCamera and a
    LinearCamera, half of the non-reference observations made by the second one.
    PARITY UNPINNED by reference vectors: Calibu is absent from the reference tree, the oracle restates the FOV
    model from its publication and pins its derivatives with central differences (tests/test_oracle_fd.py); this test
    checks the HIP path against that restatement, not against Calibu."""
    po = oracle_lib
    sc = scene.make_scene(40, 120, 6, lm_dim=lm_dim, seed=31, outlier_frac=0.0)
    z_pin = sc.obs_z.copy()
    scene.to_fov_camera(sc, 0.93)
    cam_id = np.zeros(len(sc.obs_pose), dtype=np.uint32)
    if rig == "fov_and_pinhole":
        nsel = sc.obs_per_landmark + (1 if lm_dim == 1 else 0)
        second = (np.arange(len(cam_id)) % nsel != 0) & (np.arange(len(cam_id)) % 2 == 1)
        cam_id[second] = 1
        sc.obs_z[second] = z_pin[second]
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0

    def build(cls, opts):
        b = cls(lm_dim, 6)
        b.Init(opts)
        b.AddCamera(sc.cam_params)
        if rig == "fov_and_pinhole":
            b.AddCamera(sc.cam_params[:4])
        b.add_poses(sc.poses, is_active=pa)
        b.add_landmarks(sc.landmarks, sc.lm_ref_pose)
        b.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm, cam_id=cam_id)
        return b
    o, h = build(po.OracleBundleAdjuster, gn_options(po, apply_results=0)), build(adjuster.BundleAdjuster, hip_options(apply_results=0))
    o.Solve(1)
    h.Solve(1)
    assert rel_err(h.S(), o.S()) < 1e-11
    assert rel_err(h.rhs(), o.rhs()) < 1e-10
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-7
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-7
    assert abs(h.summary().proj_error - o.summary().proj_error) < 1e-10 * o.summary().proj_error
    o, h = build(po.OracleBundleAdjuster, gn_options(po)), build(adjuster.BundleAdjuster, hip_options())
    e0 = None
    for it in range(3):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result == 0, it
        assert abs(so.proj_error - sh.proj_error) < 1e-7 * so.proj_error, it
        e0 = so.proj_error if e0 is None else e0
    assert so.proj_error < e0
    assert rel_err(h.poses()[0], o.poses()[0]) < 1e-7
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-7


def test_poses_without_residuals_and_empty_landmarks(oracle_lib):
    po = oracle_lib
    sc = scene.make_scene(30, 40, 4, lm_dim=3, seed=12)
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, apply_results=0)),
                      (adjuster.BundleAdjuster, hip_options(apply_results=0))):
        b = cls(3, 6)
        b.Init(opts)
        fill(b, sc)
        # an extra pose with no constraints (fully regularised, BundleAdjuster.cpp:1252-1258)
        b.AddPose(sc.poses[3] + np.array([0.1, 0, 0, 0, 0, 0, 0]))
        # a landmark nobody observes
        b.AddLandmark(np.array([1.0, 2.0, 3.0, 1.0]), 0, 0, True)
        b.Solve(1)
        objs.append(b)
    o, h = objs
    assert rel_err(h.S(), o.S()) < 1e-12
    assert rel_err(h.rhs(), o.rhs()) < 1e-11
    n = o.num_pose_params()
    assert h.S()[n - 1, n - 1] == 1e6


# ---- the C++ host class used directly by a C++ application ---------------------------------
@pytest.mark.parametrize("mode", [None, "--calibrate-intrinsics", "--calibrate-extrinsics", "--calibrate-fov"])
def test_cpp_application_runs_on_the_engine(mode):
    """applications/visual_ba_demo: plain C++ against include/ba/BundleAdjuster.h — the visual
    adjuster and the self-calibration instantiations <1, 6, 4, false> / <1, 6, 0, true> /
    SelfCalBundleAdjuster = <1, 6, 5> on a FovCamera."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ba_amd", "lib", "visual_ba_demo")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe] + ([mode] if mode else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "proj error" in r.stdout


def test_cpp_application_joins_the_native_communicator(tmp_path):
    """applications/visual_ba_demo --ranks 1 --rank 0 --comm-id-file F: a plain C++ program on the class's
    SetCommunicator — id created and published by rank 0, the engine-owned RCCL communicator joined inside Solve(),
    the reduced solve distributed (one rank on this box; on a node: one process per GPU with --rank R --device R)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ba_amd", "lib", "visual_ba_demo")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe, "--ranks", "1", "--rank", "0", "--comm-id-file", str(tmp_path / "comm.id")],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reduced solve distributed over the communicator" in r.stdout and "proj error" in r.stdout
    plain = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    # the same scene without a communicator ends at the same error
    last = lambda out: [ln for ln in out.splitlines() if ln.startswith("proj error")][-1]
    assert last(r.stdout).split("worst")[0] == last(plain.stdout).split("worst")[0] or \
        abs(float(last(r.stdout).split("after 9 ")[1].split(",")[0]) - float(last(plain.stdout).split("after 9 ")[1].split(",")[0])) < 1e-6


def test_pose_graph_application_with_interpolation_buffer(oracle_lib, tmp_path):
    """applications/unary_binary_imu_test — the reference's GPS + IMU pose-graph program
    (BundleAdjuster<double,0,9,0>, `ODO` / `UTM` / `IMU` log parser, gyro dead reckoning, unary
    constraints at the fixes, IMU residuals over InterpolationBufferT::GetRange, Solve(25, 0.2)) on the
    committed synthetic log.dat.  The program dumps the graph it built; the same graph goes through
    the oracle with the same options and the two solutions must agree."""
    import subprocess
    po = oracle_lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ba_amd", "lib", "unary_binary_imu_test")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    log = os.path.join(root, "applications", "unary_binary_imu_test", "log.dat")
    graph = str(tmp_path / "graph.txt")
    r = subprocess.run([exe, log, "--dump-graph", graph], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    nodes = np.array([[float(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("NODE")])
    summ = [ln for ln in r.stdout.splitlines() if ln.startswith("SUMMARY")][0].split()
    assert len(nodes) == 41   # one node per UTM record of the committed log
    # ---- the same graph through the oracle ----
    o = po.OracleBundleAdjuster(0, 9)
    opt = po.default_options()
    opt.trust_region_size = 100000
    o.Init(opt)
    o.SetGravity([0.0, 0.0, 9.8])
    cov = np.diag([1000.0, 1000.0, 30000.0, np.finfo(float).max, np.finfo(float).max, np.finfo(float).max])
    with open(graph) as f:
        lines = f.read().splitlines()
    i = 0
    nimu = 0
    while i < len(lines):
        w = lines[i].split()
        if w[0] == "POSE":
            assert o.AddPose([float(x) for x in w[3:10]], True, float(w[2])) == int(w[1])
        elif w[0] == "UNARY":
            o.AddUnaryConstraint(int(w[1]), [float(w[2]), float(w[3]), float(w[4]), 0, 0, 0, 1], cov, True)
        elif w[0] == "IMU":
            n = int(w[3])
            meas = np.array([[float(x) for x in lines[i + 1 + k].split()] for k in range(n)])
            o.AddImuResidual(int(w[1]), int(w[2]), meas)
            i += n
            nimu += 1
        i += 1
    assert nimu == len(nodes) - 1
    o.Solve(25, 0.2)
    so = o.summary()
    assert int(summ[2]) == so.result
    t_o, v_o, _ = o.poses()
    assert rel_err(nodes[:, 2:9], t_o) < 1e-6          # poses (north_star tolerance on the state)
    assert np.abs(nodes[:, 9:12] - v_o).max() < 1e-6 * max(1.0, np.abs(v_o).max())
    # the inertial error at the solution is a 1e-7 remnant of cancelling terms: absolute agreement
    assert abs(float(summ[6]) - so.inertial_error) <= 1e-8
    # (the unary weights compound over the 25 iterations, BundleAdjuster.cpp:1469: looser than the state)
    assert abs(float(summ[4]) - so.unary_error) <= 1e-3 * so.unary_error
    # the solve did something: the nodes moved away from pure gyro dead reckoning
    assert np.abs(nodes[:, 2:4]).max() > 10.0


# ---- landmark sharding on one device ------------------------------------------
def _run_engine_steps(eng, iters, out, key):
    try:
        res = []
        for _ in range(iters):
            e0 = eng.linearize()
            rc = eng.solve_gn()
            if len(res) == 0:
                out[(key, "delta_p")] = eng.get_delta_gn()[0]
            nrm = eng.compose_step(0.0, 1.0)
            pre = eng.eval_residuals()
            eng.apply_step()
            post = eng.eval_residuals()
            if post.total() > pre.total():
                eng.rollback()
            res.append((rc, e0.proj_error, pre.total(), post.total(), nrm.step_p_norm, nrm.step_l_norm))
        out[key] = res
    except Exception as exc:  # surfaced by the assertions below
        out[key] = exc


def _oracle_gn_run(po, sc, lm_dim, pa, iters):
    """The oracle on the same scene: per iteration (result, proj_error, delta_norm), the first
    pose step and the final poses — the CPU side of the sharded / distributed tests."""
    o = po.OracleBundleAdjuster(lm_dim, 6)
    o.Init(gn_options(po))
    fill(o, sc, active=pa)
    rows, dp0 = [], None
    for it in range(iters):
        o.Solve(1)
        so = o.summary()
        rows.append((so.result, so.proj_error, so.delta_norm))
        if it == 0:
            dp0 = o.delta_p()
    return rows, dp0, o.poses()[0], o.landmarks()


def _check_against_oracle(ref, out, key, poses, tol_dp=1e-8):
    rows, dp0, poses_o, _ = ref
    assert rel_err(out[(key, "delta_p")], dp0) < tol_dp          # north_star: 1e-6 on delta_x
    for it, (res_o, err_o, dn_o) in enumerate(rows):
        rc, _, pre, post, np_, nl_ = out[key][it]
        assert rc == 0
        if adjuster.RESULT_NAMES[res_o] != "Success":
            continue  # a converged scene rejects on the last bit of two equal sums
        assert post <= pre
        assert abs(post - err_o) <= 1e-8 * err_o                   # accepted error of the iteration
        assert abs((np_ + nl_) - dn_o) <= 1e-7 * max(dn_o, 1e-12)
    assert rel_err(poses, poses_o) < 1e-8


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_two_shards_equal_one(oracle_lib, lm_dim):
    """The same scene solved by ONE engine and by TWO engines holding half of the landmarks
    each (threads + in-process all-reduce hook): S, rhs, Huber median, errors, steps and
    the final state must agree — the 8-GPU path of bench.py, emulated on one GPU."""
    import threading

    from ba_amd import sharding
    sc = scene.make_scene(40, 200, 6, lm_dim=lm_dim, seed=61)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    nsel = sc.obs_per_landmark + (1 if lm_dim == 1 else 0)
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    if lm_dim == 1:
        keep[::nsel] = False

    def make(lo, hi):
        sel = keep & (sc.obs_lm >= lo) & (sc.obs_lm < hi)
        eng = hipapi.Engine(lm_dim, 6)
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks[lo:hi], sc.lm_ref_pose[lo:hi])
        eng.set_projection_residuals(sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel] - lo)
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        return eng

    L = sc.num_landmarks
    single = make(0, L)
    out = {}
    _run_engine_steps(single, 3, out, "single")
    shards = sharding.landmark_shards(np.full(L, sc.obs_per_landmark), 2)
    engs = [make(*shards[r]) for r in range(2)]
    ar = sharding.ThreadAllReduce(2)
    for r in range(2):
        engs[r].set_allreduce(ar.hook(r), r, 2)
    th = [threading.Thread(target=_run_engine_steps, args=(engs[r], 3, out, r)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not ar.failed
    for k in ("single", 0, 1):
        assert not isinstance(out[k], Exception), out[k]
    for it in range(3):
        a, b0, b1 = out["single"][it], out[0][it], out[1][it]
        assert b0 == b1 or np.allclose(b0, b1, rtol=1e-12)  # both ranks see the same sums
        assert a[0] == b0[0] == 0
        for x, y in zip(a[1:], b0[1:]):
            assert abs(x - y) <= 1e-9 * max(abs(x), 1e-12)
    ps, _, _ = single.get_poses(sc.num_poses)
    p0, _, _ = engs[0].get_poses(sc.num_poses)
    p1, _, _ = engs[1].get_poses(sc.num_poses)
    assert rel_err(p0, ps) < 1e-9 and np.array_equal(p0, p1)
    # ... and with the oracle (not only with the engine itself): first pose step, accepted errors,
    # step norms, final poses and landmarks
    ref = _oracle_gn_run(oracle_lib, sc, lm_dim, pa, 3)
    _check_against_oracle(ref, out, "single", ps)
    _check_against_oracle(ref, out, 0, p0)
    for e_ in engs + [single]:
        e_.end_solve()
    assert rel_err(np.concatenate([engs[r].get_landmarks(shards[r][1] - shards[r][0]) for r in range(2)]),
                   ref[3]) < 1e-8
    lms = np.concatenate([engs[r].get_landmarks(shards[r][1] - shards[r][0]) for r in range(2)])
    assert rel_err(lms, single.get_landmarks(L)) < 1e-9


@pytest.mark.parametrize("nranks,layout,kout", [(2, "auto", 4), (3, "auto", 4), (4, "auto", 4), (8, "auto", 4), (8, "row", 4),
                                               (8, "auto", 3), (4, "auto", 5), (4, "tri_refused", 4)],
                         ids=["2_tri", "3_col", "4_grid", "8_tri", "8_row", "8_tri_odd_blocks", "4_grid_ragged", "4_tri_refused"])
def test_distributed_solve_matches_single(oracle_lib, monkeypatch, nranks, layout, kout):
    """Distributed reduced solve (ba_hip_set_collectives; ba_amd/csrc/dist_plan.h): 300 poses -> 28 tiles
    = 7 x 7 blocks of 4 x 4 tiles owned by 2 / 3 / 4 / 8 engines (thread-emulated ranks on one GPU) that
    hold a landmark shard each; reduce-scatter of S onto the block owners, per-panel square broadcast,
    urgent + side point-to-point rows, owner-filtered trailing updates, distributed backward
    substitution.  Errors, step norms and the final state must agree with ONE engine solving the whole
    scene and with the oracle; the step is bitwise equal across the ranks; the bytes every rank moved equal
    what the message plan says (ba_hip_get_comm_stats against ba_hip_dist_plan_stats)."""
    import threading

    from ba_amd import sharding
    if layout == "tri_refused":
        # a layout that does not exist for this rank count is an error, not a silent fallback
        monkeypatch.setenv("BA_HIP_DIST_LAYOUT", "tri")
        with pytest.raises(ValueError):
            hipapi.dist_plan_stats(28, None, nranks, "tri")
        return
    if layout != "auto":
        monkeypatch.setenv("BA_HIP_DIST_LAYOUT", layout)
    # blocks of 4 tiles (the engine's choice at this size: 7 x 7 blocks), 3 (odd: no 128-blocks, 10 block rows,
    # the last one ragged) or 5 (6 block rows, the last one of 3 tiles)
    monkeypatch.setenv("BA_HIP_KOUT", str(kout))
    lm_dim = 1
    sc = scene.make_scene(300, 3000, 6, lm_dim=lm_dim, seed=67)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    nsel = sc.obs_per_landmark + 1
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::nsel] = False

    def make(lo, hi):
        sel = keep & (sc.obs_lm >= lo) & (sc.obs_lm < hi)
        eng = hipapi.Engine(lm_dim, 6)
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks[lo:hi], sc.lm_ref_pose[lo:hi])
        eng.set_projection_residuals(sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel] - lo)
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        return eng

    L = sc.num_landmarks
    single = make(0, L)
    out = {}
    iters = 3
    _run_engine_steps(single, iters, out, "single")
    shards = sharding.landmark_shards(np.full(L, sc.obs_per_landmark), nranks)
    engs = [make(*shards[r]) for r in range(nranks)]
    ar = sharding.ThreadAllReduce(nranks)
    for r in range(nranks):
        engs[r].set_allreduce(ar.hook(r), r, nranks)
        engs[r].set_collectives(ar.collectives(r))
        assert engs[r].solve_is_distributed()
    assert not single.solve_is_distributed()
    th = [threading.Thread(target=_run_engine_steps, args=(engs[r], iters, out, r)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not ar.failed
    for k in ["single"] + list(range(nranks)):
        assert not isinstance(out[k], Exception), out[k]
    for it in range(iters):
        a = out["single"][it]
        for r in range(nranks):
            b = out[r][it]
            assert a[0] == b[0] == 0
            for x, y in zip(a[1:], b[1:]):
                assert abs(x - y) <= 1e-8 * max(abs(x), 1e-12)
    ps, _, _ = single.get_poses(sc.num_poses)
    p0, _, _ = engs[0].get_poses(sc.num_poses)
    for r in range(nranks):
        pr, _, _ = engs[r].get_poses(sc.num_poses)
        assert rel_err(pr, ps) < 1e-9
        assert np.array_equal(pr, p0)  # every rank computes the same step bit for bit
        assert np.array_equal(out[(r, "delta_p")], out[(0, "delta_p")])
    # the distributed factorisation against the ORACLE's dense LDL^T on the whole scene
    ref = _oracle_gn_run(oracle_lib, sc, lm_dim, pa, iters)
    _check_against_oracle(ref, out, "single", ps)
    for r in range(nranks):
        _check_against_oracle(ref, out, r, engs[r].get_poses(sc.num_poses)[0])
    # byte accounting: what the ranks received, summed, is what the plan says for this pattern
    nzL = single.factor_tile_pattern()
    plan = hipapi.dist_plan_stats(nzL.shape[0], nzL, nranks, layout, kout)
    cs = [engs[r].comm_stats() for r in range(nranks)]
    assert all(c["factorisations"] == iters for c in cs)
    chain_recv = sum(c["chain_bytes_recv"] for c in cs)
    side_recv = sum(c["side_bytes_recv"] for c in cs)
    assert chain_recv == pytest.approx(iters * plan["chain_recv_total"], rel=1e-12)
    assert side_recv == pytest.approx(iters * plan["side_recv_total"], rel=1e-12)
    assert max(c["chain_bytes_recv"] + c["side_bytes_recv"] for c in cs) == pytest.approx(iters * plan["recv_max"], rel=1e-12)
    assert sum(c["side_bytes_sent"] for c in cs) == pytest.approx(iters * plan["side_sent_total"], rel=1e-12)
    for e_ in engs + [single]:
        e_.end_solve()
        e_.close()


def test_sparse_exchange_of_S_moves_less_with_shards_along_the_trajectory(oracle_lib):
    """The partial S of a landmark shard reaches the owners of its tile blocks point to point, and only the
    (row tile x panel) rectangles the shard's own pattern touches travel (dist_scatter_S_sparse).  Four emulated
    ranks, the same scene dealt two ways: shards contiguous in the generator's spatially random landmark id touch
    every pose pair; shards dealt along the trajectory (landmarks by reference pose) touch a band.  Both must
    reproduce the single engine; the second must move clearly fewer bytes.  (BA_HIP_DENSE_SCATTER=1, one
    reduce-scatter of the union pattern, is the fallback path and is run too.)"""
    import threading

    from ba_amd import sharding
    lm_dim, nranks = 1, 4
    sc = scene.make_scene(300, 3000, 6, lm_dim=lm_dim, seed=67)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::sc.obs_per_landmark + 1] = False
    L = sc.num_landmarks

    def make(ids):
        new_id = np.full(L, -1, dtype=np.int64)
        new_id[ids] = np.arange(len(ids))
        sel = keep & (new_id[sc.obs_lm] >= 0)
        eng = hipapi.Engine(lm_dim, 6)
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks[ids], sc.lm_ref_pose[ids])
        eng.set_projection_residuals(sc.obs_z[sel], sc.obs_pose[sel], new_id[sc.obs_lm[sel]].astype(np.uint32))
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        return eng

    single = make(np.arange(L))
    out = {}
    _run_engine_steps(single, 2, out, "single")
    ps, _, _ = single.get_poses(sc.num_poses)
    deals = {"id": [np.arange(lo, hi) for lo, hi in sharding.landmark_shards(np.full(L, sc.obs_per_landmark), nranks)],
             "trajectory": sharding.landmark_shards_along_trajectory(sc.lm_ref_pose, np.full(L, sc.obs_per_landmark), nranks)}
    assert sorted(np.concatenate(deals["trajectory"]).tolist()) == list(range(L))
    moved = {}
    for name, env in (("id", None), ("trajectory", None), ("trajectory_dense", "1")):
        if env:
            os.environ["BA_HIP_DENSE_SCATTER"] = env
        try:
            engs = [make(deals[name.split("_")[0]][r]) for r in range(nranks)]
            ar = sharding.ThreadAllReduce(nranks)
            for r in range(nranks):
                engs[r].set_allreduce(ar.hook(r), r, nranks)
                engs[r].set_collectives(ar.collectives(r))
            th = [threading.Thread(target=_run_engine_steps, args=(engs[r], 2, out, (name, r))) for r in range(nranks)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=300)
            assert not ar.failed
        finally:
            os.environ.pop("BA_HIP_DENSE_SCATTER", None)
        for r in range(nranks):
            assert not isinstance(out[(name, r)], Exception), out[(name, r)]
            pr, _, _ = engs[r].get_poses(sc.num_poses)
            assert rel_err(pr, ps) < 1e-9
            for a, b in zip(out["single"], out[(name, r)]):
                assert a[0] == b[0] == 0
                for x, y in zip(a[1:], b[1:]):
                    assert abs(x - y) <= 1e-8 * max(abs(x), 1e-12)
        moved[name] = sum(e_.comm_stats()["reduce_scatter_bytes"] for e_ in engs)
        for e_ in engs:
            e_.end_solve()
            e_.close()
    assert moved["trajectory"] < 0.7 * moved["id"], moved
    assert moved["trajectory"] < moved["trajectory_dense"], moved
    single.end_solve()
    single.close()


def test_tile_sparse_factorisation_matches_oracle(oracle_lib):
    """300 poses (n = 1788, 28 tiles of 64): poses far apart on the loop share no landmark, so S
    has structurally zero 64x64 tiles and the factorisation skips tile products (symbolic
    pattern, k_chol.hip).  The step must still agree with the oracle's dense LDL^T, and with
    the engine's own dense path (BA_HIP_DENSE is read once per process, so the dense reference
    here is the stand-alone dense solver on the tapped S)."""
    po = oracle_lib
    sc = scene.make_scene(300, 6000, 6, lm_dim=1, seed=23)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, 1, active=pa, apply_results=0, use_triangular_matrices=0)
    o.Solve(1)
    h.Solve(1)
    s = h.S()
    n = s.shape[0]
    nt = (n + 63) // 64
    tiles = np.zeros((nt, nt), dtype=bool)
    for a in range(nt):
        for b in range(nt):
            tiles[a, b] = np.any(s[64 * a:64 * a + 64, 64 * b:64 * b + 64] != 0.0)
    assert tiles.mean() < 0.8, "the scene is supposed to have structurally zero tiles"
    assert rel_err(s, o.S()) < 1e-12
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-8
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-8
    eng = hipapi.Engine(1, 6)
    x, rc = eng.dense_solve(s, h.rhs())
    assert rc == 0 and rel_err(h.delta_p(), x) < 1e-9


@pytest.mark.parametrize("variant", ["damped", "increase_allowed", "no_robust_norm", "exit_tests", "exit_tests_dogleg"])
def test_solve_arguments_and_exit_tests(oracle_lib, variant):
    """Solve()'s arguments and the exit tests of BundleAdjuster.cpp:648-661 (Q14, Q15 defaults):
    gn_damping (:1108-1110), error_increase_allowed (:1134), the robust norm switch (:1374),
    and the default thresholds (error change 0.01, parameter change 1e-3) that end the loop with
    ErrorChangeBelowThreshold / ParamChangeBelowThreshold — the result code, the number of
    iterations that ran (visible in the state) and the state itself must follow the oracle."""
    po = oracle_lib
    sc = scene.make_scene(24, 90, 5, lm_dim=1, seed=47)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    okw, hkw, args = {}, {}, {}
    if variant == "damped":
        args = dict(gn_damping=0.5)
    elif variant == "increase_allowed":
        args = dict(gn_damping=2.5, error_increase_allowed=True)  # overshoots; the step is kept anyway
    elif variant == "no_robust_norm":
        okw = hkw = dict(use_robust_norm_for_proj_residuals=0)
    oo = gn_options(po, **okw)
    ho = hip_options(**hkw)
    if variant.startswith("exit_tests"):
        for opt in (oo, ho):  # the reference's defaults (BundleAdjuster.h:85-86)
            opt.error_change_threshold = 0.01
            opt.param_change_threshold = 1e-3
            opt.use_dogleg = 1 if variant.endswith("dogleg") else 0
    o = po.OracleBundleAdjuster(1, 6)
    o.Init(oo)
    h = adjuster.BundleAdjuster(1, 6)
    h.Init(ho)
    fill(o, sc, active=pa)
    fill(h, sc, active=pa)
    iters = 12 if variant.startswith("exit_tests") else (2 if variant == "increase_allowed" else 3)
    o.Solve(iters, **args)
    h.Solve(iters, **args)
    so, sh = o.summary(), h.summary()
    assert so.result == sh.result
    if variant.startswith("exit_tests"):
        assert so.result in (2, 3)  # ErrorChangeBelowThreshold / ParamChangeBelowThreshold
    assert abs(so.proj_error - sh.proj_error) <= 1e-8 * max(so.proj_error, 1e-12)
    assert abs(so.delta_norm - sh.delta_norm) <= 1e-6 * max(so.delta_norm, 1e-9)
    _state_close(o, h, 1e-7)


@pytest.mark.parametrize("pose_dim", [6, 15])
def test_regularize_pose_and_root_pose(oracle_lib, pose_dim):
    """Gauge handling of BuildProblem (:1237-1330, a3): RegularizePose on chosen poses (Q8: the
    rotation flag masks indices 2,4,5), a non-default root pose (SetRootPoseId) under automatic
    regularisation with every pose active, velocities / biases in the state for PoseSize 15
    (gravity-axis regularisation, bias regularisation).  Masked parameters carry 1e6 on the
    diagonal of S (Q12) and stay put."""
    po = oracle_lib
    P = 18
    sc = scene.make_scene(P, 70, 5, lm_dim=1, seed=53)
    if pose_dim == 15:
        scene.add_inertial(sc, period=60.0 * P / 100.0)
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po)), (adjuster.BundleAdjuster, hip_options())):
        b = cls(1, pose_dim)
        b.Init(opts)
        if pose_dim == 15:
            b.SetGravity(sc.gravity)
        fill(b, sc)  # all poses active: the gauge comes from the masks alone
        if pose_dim == 15:
            for i in range(P - 1):
                b.AddImuResidual(i, i + 1, sc.imu_meas[i])
        b.SetRootPoseId(5)
        b.RegularizePose(2, True, False, False, False)    # translation
        b.RegularizePose(9, False, False, False, True)    # "rotation": indices 2, 4, 5
        b.RegularizePose(12, True, pose_dim == 15, pose_dim == 15, True)
        objs.append(b)
    o, h = objs
    p_before = h.poses()[0].copy()
    for it in range(2):
        o.Solve(1)
        h.Solve(1)
        assert o.summary().result == h.summary().result
        if it == 0:
            assert rel_err(h.S(), o.S()) < 1e-9
            assert rel_err(h.rhs(), o.rhs()) < 1e-9
            d = np.diag(h.S())
            assert (d == 1e6).sum() >= 3 + 3 + 3  # the masks put 1e6 on the diagonal
    _state_close(o, h, 1e-6)
    p_after = h.poses()[0]
    assert np.array_equal(p_after[2, :3], p_before[2, :3])  # translation of pose 2 held fixed


@pytest.mark.parametrize("variant", ["robust_inertial", "biases_in_batch", "imu_weights", "imu_sigmas", "imu_noise_vectors"])
def test_visual_inertial_options(oracle_lib, variant):
    """Options of the inertial path (BundleAdjuster.h:72-107, BundleAdjuster.cpp:1494-1541):
    Huber weighting of the IMU residuals, regularize_biases_in_batch, per-residual weights of
    AddImuResidual, non-default gyro / accelerometer sigmas in the covariance propagation."""
    po = oracle_lib
    P = 16
    sc = scene.make_scene(P, 60, 5, lm_dim=1, seed=57)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    kw = {}
    if variant == "robust_inertial":
        kw = dict(use_robust_norm_for_inertial_residuals=1)
    elif variant == "biases_in_batch":
        kw = dict(regularize_biases_in_batch=1)
    elif variant == "imu_sigmas":
        kw = dict(gyro_sigma=2e-4, accel_sigma=5e-3, gyro_bias_sigma=1e-5, accel_bias_sigma=2e-4)
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, **kw)), (adjuster.BundleAdjuster, hip_options(**kw))):
        b = cls(1, 15)
        b.Init(opts)
        b.SetGravity(sc.gravity)
        fill(b, sc)
        if variant == "imu_noise_vectors":  # SetImuCalibration: anisotropic r / r_b instead of the option sigmas
            b.SetImuNoise(1e-9 * np.array([1.0, 2.0, 4.0, 900.0, 1500.0, 2500.0]),
                          1e-12 * np.array([1.0, 3.0, 2.0, 50.0, 80.0, 20.0]))
        for i in range(P - 1):
            b.AddImuResidual(i, i + 1, sc.imu_meas[i], 0.25 + 0.1 * i if variant == "imu_weights" else 1.0)
        objs.append(b)
    o, h = objs
    for it in range(2):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        if it == 0:
            assert rel_err(h.S(), o.S()) < 1e-9
            assert rel_err(h.rhs(), o.rhs()) < 1e-9
        assert abs(so.inertial_error - sh.inertial_error) <= 1e-6 * max(so.inertial_error, 1e-12)
    _state_close(o, h, 1e-6)


def test_get_projection_residual(oracle_lib):
    """GetProjectionResidual(id) after a Solve() (reference BundleAdjuster.h:568-571,
    BundleAdjuster.cpp:155-181): ids, measurement, Huber weight and the residual vector z - pi at
    the state the solve left behind, against the oracle's per-residual records."""
    po = oracle_lib
    sc = scene.make_scene(15, 50, 5, lm_dim=1, seed=59)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, 1, active=pa)
    o.Solve(2)
    h.Solve(2)
    assert o.summary().result == h.summary().result == 0
    r_o, w_o = o.proj_residuals(), o.proj_weights()
    acc = accepted_obs(sc)
    n = h.GetNumProjResiduals()
    assert n == len(acc) == len(w_o)
    for rid in list(range(0, n, 7)) + [n - 1]:
        r = h.GetProjectionResidual(rid)
        assert (r["x_meas_id"], r["x_ref_id"], r["landmark_id"]) == acc[rid]
        assert np.allclose(r["residual"], r_o[rid], rtol=0, atol=1e-7 * max(1.0, np.abs(r_o[rid]).max()))
        assert abs(r["weight"] - w_o[rid]) <= 1e-9 * max(w_o[rid], 1e-12)
        assert abs(r["mahalanobis_distance"] - (r_o[rid] ** 2).sum() * w_o[rid]) <= 1e-6 * max(1.0, (r_o[rid] ** 2).sum())
        assert r["orig_weight"] == 1.0


def test_incremental_use_add_then_solve_again(oracle_lib):
    """The reference's incremental pattern ("Solve may be called repeatedly after
    more Add* calls"): solve with the first 40 landmarks, add 40 more landmarks with their
    observations, solve again.  Ids continue, the state of the first Solve() is kept, and the
    second one must track the oracle."""
    po = oracle_lib
    sc = scene.make_scene(20, 80, 5, lm_dim=1, seed=43)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    first = sc.obs_lm < 40
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po)), (adjuster.BundleAdjuster, hip_options())):
        b = cls(1, 6)
        b.Init(opts)
        b.AddCamera(sc.cam_params)
        b.add_poses(sc.poses, is_active=pa)
        b.add_landmarks(sc.landmarks[:40], sc.lm_ref_pose[:40])
        b.add_projection_residuals(sc.obs_z[first], sc.obs_pose[first], sc.obs_lm[first])
        objs.append(b)
    o, h = objs
    o.Solve(2)
    h.Solve(2)
    _state_close(o, h)
    for b in objs:
        b.add_landmarks(sc.landmarks[40:], sc.lm_ref_pose[40:])
        ids = b.add_projection_residuals(sc.obs_z[~first], sc.obs_pose[~first], sc.obs_lm[~first])
        assert b.GetNumLandmarks() == 80
    o.Solve(2)
    h.Solve(2)
    so, sh = o.summary(), h.summary()
    assert so.result == sh.result
    assert abs(so.proj_error - sh.proj_error) <= 1e-9 * so.proj_error
    _state_close(o, h)
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-8


def test_landmark_reliability_and_outlier_ratio(oracle_lib):
    """Q9 (BundleAdjuster.cpp:127-134): an inverse depth that would turn negative is reverted and
    the landmark flagged unreliable; LandmarkOutlierRatio counts residuals above
    projection_outlier_threshold (:184-186).  Far landmarks with noisy observations trigger both;
    flags and ratios must agree with the oracle landmark by landmark."""
    po = oracle_lib
    sc = scene.make_scene(25, 120, 5, lm_dim=1, seed=29)
    rng = np.random.default_rng(3)
    # push a third of the landmarks far away (tiny inverse depth) and perturb their observations
    lms = sc.landmarks.copy()
    far = rng.choice(sc.num_landmarks, sc.num_landmarks // 3, replace=False)
    centre = sc.poses[:, :3].mean(axis=0)
    lms[far, :3] = centre + (lms[far, :3] - centre) * 200.0
    sc.landmarks = lms
    sc.obs_z = sc.obs_z + rng.normal(0, 20.0, sc.obs_z.shape)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, 1, active=pa, projection_outlier_threshold=4.0)
    for _ in range(3):
        o.Solve(1)
        h.Solve(1)
        assert o.summary().result == h.summary().result
    rel_o = np.array([o.IsLandmarkReliable(i) for i in range(sc.num_landmarks)])
    rel_h = np.array([h.IsLandmarkReliable(i) for i in range(sc.num_landmarks)])
    out_o = np.array([o.LandmarkOutlierRatio(i) for i in range(sc.num_landmarks)])
    out_h = np.array([h.LandmarkOutlierRatio(i) for i in range(sc.num_landmarks)])
    assert (~rel_o).sum() > 0, "the scene is supposed to produce unreliable landmarks"
    assert out_o.max() > 0
    assert np.array_equal(rel_o, rel_h)
    assert np.allclose(out_o, out_h, rtol=0, atol=1e-12)
    _state_close(o, h, 1e-7)


def test_reduced_camera_matrix_dump(tmp_path, monkeypatch):
    """write_reduced_camera_matrix (BundleAdjuster.cpp:600-606): s.txt / rhs.txt in the
    reference's CSV format reproduce the tapped S and rhs to the printed precision."""
    sc = scene.make_scene(12, 40, 4, lm_dim=1, seed=11)
    monkeypatch.chdir(tmp_path)
    h = adjuster.BundleAdjuster(1, 6)
    h.Init(hip_options(write_reduced_camera_matrix=2))
    fill(h, sc)
    h.Solve(1)
    s = np.loadtxt(tmp_path / "s.txt", delimiter=",")
    rhs = np.loadtxt(tmp_path / "rhs.txt", delimiter=",")
    assert s.shape == h.S().shape and rel_err(s, h.S()) < 1e-15
    assert rel_err(rhs, h.rhs()) < 1e-15
    first = (tmp_path / "s.txt").read_text().splitlines()[0]
    assert ", " in first and ";" not in first  # Utils.h:66 kLongCsvFmt


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_jacobian_dumps_and_loader(oracle_lib, tmp_path, monkeypatch, lm_dim):
    """j_pr.txt / r_pr.txt / j_l.txt (BundleAdjuster.cpp:608-616) + ba_amd/dumps.py: the dumped
    Jacobians equal the oracle's sqrt(w) J blocks, and s.txt / rhs.txt equal the Schur complement
    rebuilt from the dumped files with dense numpy — what a third party holding a build of the
    original would diff."""
    from ba_amd import dumps
    po = oracle_lib
    sc = scene.make_scene(14, 50, 5, lm_dim=lm_dim, seed=19)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    la[[3, 17]] = 0
    monkeypatch.chdir(tmp_path)
    o, h = both(po, sc, lm_dim, active=pa, lm_active=la, apply_results=0, write_reduced_camera_matrix=2)
    o.Solve(1)
    h.Solve(1)
    d = dumps.load_reduced_system(str(tmp_path))
    assert set(d) == {"s", "rhs", "j_pr", "r_pr", "j_l"}
    O = h.GetNumProjResiduals()
    nP, nL = int(pa.sum()), int(la.sum())
    assert d["j_pr"].shape == (2 * O, 6 * nP) and d["j_l"].shape == (2 * O, lm_dim * nL) and d["r_pr"].shape == (2 * O,)
    err_s, err_r = dumps.check_consistency(d, lm_dim)
    assert err_s < 1e-11 and err_r < 1e-11, (err_s, err_r)
    # against the oracle: its per-residual Jacobians are unweighted (as stored in the residual), the
    # dumped matrices carry sqrt(w) (j_pr_ entries, :1636-1642)
    jm_o, jr_o, jl_o = o.proj_jacobians()
    sw = np.sqrt(o.proj_weights())
    acc = accepted_obs(sc)
    popt = -np.ones(sc.num_poses, dtype=int)
    popt[pa > 0] = np.arange(nP)
    lopt = -np.ones(sc.num_landmarks, dtype=int)
    lopt[la > 0] = np.arange(nL)
    Jp, Jl = np.zeros_like(d["j_pr"]), np.zeros_like(d["j_l"])
    for a, (pm, pr, l) in enumerate(acc):
        listed = lm_dim != 1 or pm != pr
        if listed and popt[pm] >= 0:
            Jp[2 * a:2 * a + 2, 6 * popt[pm]:6 * popt[pm] + 6] += sw[a] * jm_o[a]
        if lm_dim == 1 and listed and popt[pr] >= 0:
            Jp[2 * a:2 * a + 2, 6 * popt[pr]:6 * popt[pr] + 6] += sw[a] * jr_o[a]
        if lopt[l] >= 0:
            Jl[2 * a:2 * a + 2, lm_dim * lopt[l]:lm_dim * lopt[l] + lm_dim] = sw[a] * jl_o[a]
    assert rel_err(d["j_pr"], Jp) < 1e-11
    assert rel_err(d["j_l"], Jl) < 1e-11
    assert rel_err(d["r_pr"], (sw[:, None] * o.proj_residuals()).ravel()) < 1e-11
    assert dumps.diff(str(tmp_path), str(tmp_path))["s"] == 0.0


# ---- full-size properties (BASELINE.json configs[1]) ---------------------------------------
def test_config2_size_properties():
    """1k poses / 100k landmarks / 1M residuals: size-independent properties —
    S delta = rhs, symmetry of the gathered blocks, determinism (bitwise), error decrease."""
    sc = scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    runs = []
    for _ in range(2):
        h = adjuster.BundleAdjuster(1, 6)
        h.Init(hip_options(apply_results=0, use_triangular_matrices=0))
        fill(h, sc, active=pa)
        h.Solve(1)
        runs.append((h.S(), h.rhs(), h.delta_p()))
    s, rhs, dp_ = runs[0]
    assert np.array_equal(s, runs[1][0]) and np.array_equal(dp_, runs[1][2])  # no atomics
    assert np.abs(s - s.T).max() <= 1e-9 * np.abs(s).max()
    assert rel_err(s @ dp_, rhs) < 1e-9
    h = adjuster.BundleAdjuster(1, 6)
    h.Init(hip_options())
    fill(h, sc, active=pa)
    h.Solve(1)
    e0 = h.summary().proj_error
    h.Solve(2)
    assert h.summary().proj_error < e0


def test_large_system_properties():
    """3000 poses (n = 17 988, 282 tiles): the regime of BASELINE.json configs[3] in the solver —
    512-column outer panels, full-occupancy XCD-swizzled bulk updates, tile-sparse skipping —
    checked through size-independent properties: S delta = rhs, symmetry, bitwise determinism,
    error decrease."""
    sc = scene.make_scene(3000, 30000, 10, lm_dim=1, seed=5)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    runs = []
    for _ in range(2):
        h = adjuster.BundleAdjuster(1, 6)
        h.Init(hip_options(apply_results=0, use_triangular_matrices=0))
        fill(h, sc, active=pa)
        h.Solve(1)
        runs.append((h.rhs(), h.delta_p(), h.S() if not runs else None))
        del h
    rhs, dp_, s = runs[0]
    assert np.array_equal(dp_, runs[1][1]) and np.array_equal(rhs, runs[1][0])
    assert np.abs(s - s.T).max() <= 1e-9 * np.abs(s).max()
    assert rel_err(s @ dp_, rhs) < 1e-9
    del s
    h = adjuster.BundleAdjuster(1, 6)
    h.Init(hip_options(write_reduced_camera_matrix=0))
    fill(h, sc, active=pa)
    h.Solve(1)
    e0 = h.summary().proj_error
    h.Solve(2)
    assert h.summary().proj_error < e0


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_config1_scale_step_matches_oracle(oracle_lib, lm_dim):
    """BASELINE.json configs[1] (1k poses / 100k landmarks / 1M residuals) against the oracle on
    the same scene: the Gauss-Newton step of the first iteration — north_star's parity bar is
    1e-6 relative on delta_x.  The oracle needs ~7 s for its dense LDL^T.  LmSize 1 (the reference's
    instantiation: inverse depth in a reference pose) and LmSize 3 (world points, north_star's 6x3 / 3x3 blocks)."""
    po = oracle_lib
    sc = scene.make_scene(1000, 100000, 10, lm_dim=lm_dim, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o, h = both(po, sc, lm_dim, active=pa, apply_results=0, write_reduced_camera_matrix=0)
    o.Solve(1)
    h.Solve(1)
    so, sh = o.summary(), h.summary()
    assert so.result == sh.result == 0
    assert abs(so.proj_error - sh.proj_error) <= 1e-10 * so.proj_error
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-6
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-6
    print("config-1 scale: delta_p rel err %.2e, delta_l rel err %.2e" %
          (rel_err(h.delta_p(), o.delta_p()), rel_err(h.delta_l(), o.delta_l())))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["config2_gn", "config4_dogleg"])
def test_visual_inertial_at_the_largest_size_the_oracle_follows(oracle_lib, kind):
    """BASELINE.json configs[2] / configs[4] at the size of bench.py's CPU-baseline sample and a bit beyond what the
    miniatures cover: 400 poses / 20k landmarks / 200k residuals + 399 IMU pre-integration residuals, PoseSize 15
    (n = 6000, 94 tiles: tile-sparse factorisation, look-ahead, k_imu in its wavefront form) — Gauss-Newton, or with
    unary priors + binary odometry and the dogleg trust region.  One Solve(1) against the oracle: result code, every
    error sum, the pose step to north_star's 1e-6, the state."""
    po = oracle_lib
    P = 400
    dog = 1 if kind == "config4_dogleg" else 0
    sc = scene.make_scene(P, 20000, 10, lm_dim=1, seed=2)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, use_dogleg=dog)),
                      (adjuster.BundleAdjuster, hip_options(use_dogleg=dog, write_reduced_camera_matrix=0))):
        b = cls(1, 15)
        b.Init(opts)
        scene.populate(b, sc, imu=True, priors=bool(dog), unary_every=20)
        objs.append(b)
    o, h = objs
    o.Solve(1)
    h.Solve(1)
    so, sh = o.summary(), h.summary()
    assert so.result == sh.result
    for name in ("proj_error", "inertial_error", "unary_error", "binary_error", "delta_norm"):
        a, b_ = getattr(so, name), getattr(sh, name)
        assert abs(a - b_) <= 1e-6 * max(abs(a), 1e-9), (name, a, b_)
    if dog:
        assert abs(so.trust_region_size - sh.trust_region_size) <= 1e-6 * abs(so.trust_region_size)
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-6
    _state_close(o, h, 1e-6)
    print("%s at n = %d: delta_p rel err %.2e" % (kind, 15 * P, rel_err(h.delta_p(), o.delta_p())))


@pytest.mark.gpu
def test_blocked_128_trailing_update_on_small_systems():
    """k_update128 (the 128x128 trailing-update kernel, its row-mode companion launch, its
    indefinite fallback and the ownership filter of the distributed solve) normally only runs on
    trailing matrices of >= 128 tiles.  BA_HIP_BULK_FULL_M is read once per process, so the solver
    tests are re-run in a child process with the threshold lowered to 16 tiles.  (The grid of explicit tile
    patterns under this and the other per-process switches lives in test_tile_factor_gpu.py.)"""
    import subprocess
    import sys
    if os.environ.get("BA_TEST_NESTED"):
        pytest.skip("nested run")
    env = dict(os.environ, BA_HIP_BULK_FULL_M="16", BA_TEST_NESTED="1")
    r = subprocess.run(
        [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
         "dense_cholesky_solve or tile_sparse or distributed_solve_matches_single or reduced_system_and_step"],
        env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("width", ["4", "3"])
def test_one_workgroup_square_factorisation(width):
    """BA_HIP_SQUARE=1 (k_square + k_rowpanel: the diagonal square of a sub-panel factorised by one workgroup;
    measured slower than the per-column chain and therefore opt-in) — the solver tests re-run in a
    child process with it switched on, at square widths 4 and 3 (ragged squares, structurally zero tiles,
    indefinite systems, the rhs row).  Widths 1 to 4 on explicit tile patterns, checked on the factor itself:
    test_tile_factor_gpu.py."""
    import subprocess
    import sys
    if os.environ.get("BA_TEST_NESTED"):
        pytest.skip("nested run")
    env = dict(os.environ, BA_HIP_SQUARE="1", BA_HIP_SQ_W=width, BA_TEST_NESTED="1")
    r = subprocess.run(
        [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
         "dense_cholesky_solve or tile_sparse or reduced_system_and_step or config1_scale_step"],
        env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("lm_dim", [1, 3])
def test_per_pose_camera_parameters(oracle_lib, lm_dim):
    """Options::use_per_pose_cam_params (reference BundleAdjuster.h:96, parallel_algos.h:54-57,
    BundleAdjuster.cpp:162-176): every residual is evaluated with the intrinsics stored on its
    measurement pose.  Engine vs oracle on one linearisation and over three iterations; equal
    per-pose parameters reproduce the rig-camera result bit for bit; a missing parameter set is an
    error, not a silent fallback."""
    po = oracle_lib
    sc = scene.make_scene(30, 60, 5, lm_dim=lm_dim, seed=7)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    rng = np.random.default_rng(3)
    pc = np.asarray(sc.cam_params)[None, :] * (1.0 + 0.03 * rng.uniform(-1, 1, (sc.num_poses, 4)))
    o, h = both(po, sc, lm_dim, active=pa, apply_results=0)
    o0, h0 = both(po, sc, lm_dim, active=pa, apply_results=0)
    for b in (o, h):
        b.SetPoseCamParams(pc)
        b.SetUsePerPoseCamParams(True)
    h0.SetPoseCamParams(np.tile(np.asarray(sc.cam_params), (sc.num_poses, 1)))
    for b in (o, h, o0, h0):
        b.Solve(1)
    assert rel_err(h.S(), o.S()) < 1e-12
    assert rel_err(h.rhs(), o.rhs()) < 1e-11
    assert rel_err(h.proj_weights(), o.proj_weights()) < 1e-12
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-8
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-8
    assert abs(h.summary().proj_error - o.summary().proj_error) < 1e-9 * o.summary().proj_error
    assert rel_err(o.S(), o0.S()) > 1e-3                  # the option is not a no-op
    hr = adjuster.BundleAdjuster(lm_dim, 6)               # rig intrinsics, no per-pose parameters
    hr.Init(hip_options(apply_results=0))
    fill(hr, sc, active=pa)
    hr.Solve(1)
    assert np.array_equal(h0.S(), hr.S()) and np.array_equal(h0.delta_p(), hr.delta_p())
    # iterations with the update applied
    o, h = both(po, sc, lm_dim, active=pa)
    for b in (o, h):
        b.SetPoseCamParams(pc)
        b.SetUsePerPoseCamParams(True)
    for _ in range(3):
        o.Solve(1)
        h.Solve(1)
        assert o.summary().result == h.summary().result
        assert abs(h.summary().proj_error - o.summary().proj_error) < 1e-8 * o.summary().proj_error
    assert rel_err(h.poses()[0], o.poses()[0]) < 1e-8
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-8
    # switching the option off again restores the rig camera
    h.SetUsePerPoseCamParams(False)
    o.SetUsePerPoseCamParams(False)
    o.Solve(1)
    h.Solve(1)
    assert abs(h.summary().proj_error - o.summary().proj_error) < 1e-8 * o.summary().proj_error


@pytest.mark.gpu
@pytest.mark.parametrize("pose_dim", [9, 15])
def test_get_imu_residual(oracle_lib, pose_dim):
    """GetImuResidual(id) (reference BundleAdjuster.h:563-565): pose ids, measurements and weight
    from the host graph, the residual vector (Types.h:654-689) read back from the device after an
    accepted step — against the oracle's ImuResidualT::residual."""
    po = oracle_lib
    P = 14
    sc = scene.make_scene(P, 60, 5, lm_dim=1, seed=53)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po)), (adjuster.BundleAdjuster, hip_options())):
        b = cls(1, pose_dim)
        b.Init(opts)
        b.SetGravity(sc.gravity)
        fill(b, sc)
        for i in range(P - 1):
            b.AddImuResidual(i, i + 1, sc.imu_meas[i], 1.0 + 0.5 * (i % 3))
        objs.append(b)
    o, h = objs
    before = h.GetImuResidual(3)
    assert before["pose1_id"] == 3 and before["pose2_id"] == 4 and before["weight"] == 1.0
    assert before["num_measurements"] == len(sc.imu_meas[3]) and not before["residual"].any()
    o.Solve(1)
    h.Solve(1)
    assert o.summary().result == h.summary().result == 0
    ro = o.imu_residuals()
    assert np.abs(ro[:, :pose_dim]).max() > 1e-6
    for i in range(P - 1):
        r = h.GetImuResidual(i)
        assert r["pose1_id"] == i and r["pose2_id"] == i + 1 and r["weight"] == 1.0 + 0.5 * (i % 3)
        assert np.abs(r["residual"][:pose_dim] - ro[i, :pose_dim]).max() < 1e-7 * max(1.0, np.abs(ro[i, :pose_dim]).max())


@pytest.mark.gpu
def test_calculate_inertial_covariance_once(oracle_lib):
    """Options::calculate_inertial_covariance_once (reference BundleAdjuster.h:106,
    parallel_algos.h:189-205): the integration covariance and the bias Jacobian of every inertial
    residual are frozen at its first linearisation — across iterations AND across Solve() calls.
    Engine vs oracle over four Solve(1) calls; the option changes the result; residuals appended
    later get their own first linearisation."""
    po = oracle_lib
    P = 16
    sc = scene.make_scene(P, 60, 5, lm_dim=1, seed=57)
    scene.add_inertial(sc, period=60.0 * P / 100.0)

    def make(cls, opts, once, n_imu):
        b = cls(1, 15)
        b.Init(opts)
        b.SetGravity(sc.gravity)
        fill(b, sc)
        b.SetCalculateInertialCovarianceOnce(once)
        for i in range(n_imu):
            b.AddImuResidual(i, i + 1, sc.imu_meas[i])
        return b

    o = make(po.OracleBundleAdjuster, gn_options(po, use_dogleg=1), True, P - 3)
    h = make(adjuster.BundleAdjuster, hip_options(use_dogleg=1), True, P - 3)
    h_off = make(adjuster.BundleAdjuster, hip_options(use_dogleg=1), False, P - 3)
    for it in range(4):
        if it == 2:  # two more residuals: linearised (and frozen) for the first time in this Solve
            for b in (o, h, h_off):
                for i in (P - 3, P - 2):
                    b.AddImuResidual(i, i + 1, sc.imu_meas[i])
        o.Solve(1)
        h.Solve(1)
        h_off.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        assert abs(so.inertial_error - sh.inertial_error) <= 1e-6 * max(so.inertial_error, 1e-12)
        assert abs(so.proj_error - sh.proj_error) <= 1e-6 * max(so.proj_error, 1e-12)
    _state_close(o, h, 1e-6)
    # the frozen covariances are not the re-computed ones
    assert abs(h.summary().inertial_error - h_off.summary().inertial_error) > 1e-9 * h.summary().inertial_error


@pytest.mark.gpu
def test_conditioning_error_sums(oracle_lib):
    """SolutionSummary::cond_proj_error / cond_inertial_error (reference BundleAdjuster.cpp:680-704):
    sums over the residuals that tie an active pose to an inactive one (BundleAdjuster.h:503-510,
    538-545) — |r|^2 of the projection residuals, Mahalanobis distance of the inertial ones."""
    po = oracle_lib
    P = 14
    sc = scene.make_scene(P, 60, 5, lm_dim=1, seed=53)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    pa = np.ones(P, dtype=np.uint8)
    pa[[0, 1]] = 0  # inactive start: its landmarks' residuals and the IMU residual 1 -> 2 condition
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, use_dogleg=1)), (adjuster.BundleAdjuster, hip_options(use_dogleg=1))):
        b = cls(1, 15)
        b.Init(opts)
        b.SetGravity(sc.gravity)
        fill(b, sc, active=pa)
        for i in range(P - 1):
            b.AddImuResidual(i, i + 1, sc.imu_meas[i])
        objs.append(b)
    o, h = objs
    for _ in range(2):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        assert so.num_cond_proj_residuals == sh.num_cond_proj_residuals > 0
        assert so.num_cond_inertial_residuals == sh.num_cond_inertial_residuals == 1
        cp, ci = h.cond_errors()
        assert so.cond_proj_error > 0 and so.cond_inertial_error > 0
        if so.result == 0:  # after a rejected step the reference's per-residual values are those of the rejected state
            assert abs(cp - so.cond_proj_error) <= 1e-6 * so.cond_proj_error
            assert abs(ci - so.cond_inertial_error) <= 1e-6 * so.cond_inertial_error


@pytest.mark.gpu
@pytest.mark.parametrize("n", [26000, 33000])
def test_dense_solve_with_1024_column_panels(n):
    """n = 33 000 (516 tiles): the schedule of BASELINE.json configs[3] — outer panels of 16 tiles,
    left-looking sub-panels of 8, k_update128 for the bulk and for the rectangle under the next
    panel — on a dense diagonally dominant matrix, checked through the residual of the solve and
    bitwise repeatability.  n = 26 000 (407 tiles): 16-tile panels with right-looking sub-panels
    of 4."""
    rng = np.random.default_rng(9)
    a = rng.random((n, n), dtype=np.float32).astype(np.float64)
    a -= 0.5
    a = np.tril(a)
    a[np.diag_indices(n)] = 0.3 * n          # strictly diagonally dominant: SPD
    b = rng.normal(size=n)
    eng = hipapi.Engine(1, 6)
    x, rc = eng.dense_solve(a, b)
    assert rc == 0
    x2, rc2 = eng.dense_solve(a, b)
    assert rc2 == 0 and np.array_equal(x, x2)
    # A x with the symmetric matrix stored as its lower triangle
    ax = a @ x
    ax += a.T @ x
    ax -= a.diagonal() * x
    assert rel_err(ax, b) < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("use_dogleg", [0, 1])
def test_landmarks_only_solve_with_all_poses_fixed(oracle_lib, lm_dim, use_dogleg):
    """Every pose inactive, landmarks active: the reference skips CalculateGn but still calls
    GetLandmarkDelta (BundleAdjuster.cpp:959-967, 1089-1106), so the landmarks move by
    delta_l = V^-1 rhs_l.  (Round-1 finding: the host class skipped the back-substitution too.)"""
    po = oracle_lib
    sc = scene.make_scene(20, 80, 6, lm_dim=lm_dim, seed=33)
    pa = np.zeros(sc.num_poses, dtype=np.uint8)
    o, h = both(po, sc, lm_dim, active=pa, use_dogleg=use_dogleg)
    lm0 = np.array(sc.landmarks, dtype=float)
    for _ in range(3):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        assert abs(so.proj_error - sh.proj_error) < 1e-9 * so.proj_error
        assert abs(so.delta_norm - sh.delta_norm) < 1e-8 * max(so.delta_norm, 1e-12)
        assert rel_err(h.delta_l(), o.delta_l()) < 1e-10
    assert np.abs(np.asarray(h.landmarks()) - lm0).max() > 1e-6   # the landmarks did move
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-10
    th, _, _ = h.poses()
    assert rel_err(th, sc.poses) < 1e-15                          # the poses did not


# ---- BASELINE.json configs at full size / all residual kinds ------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nranks", [2, 4])
def test_config4_miniature_on_landmark_shards_with_distributed_solve(oracle_lib, monkeypatch, nranks):
    """The 8-GPU form of BASELINE.json configs[4], in miniature and on emulated ranks: reprojection residuals
    sharded by landmark, IMU + unary priors + binary odometry on rank 0 only, PoseSize 15, dogleg trust region,
    gauge masks from GLOBAL counts, and the reduced solve DISTRIBUTED over the ranks (SetAllReduce +
    SetCollectives: what bench.py --gpus N --config 4 does through SetCommunicator).  n = 80 x 15 = 1200 -> 19 tiles,
    blocks of 2 tiles.  Three Solve(1) calls per rank against the oracle on the whole scene: result codes, every
    error sum, the trust region, the state; the ranks agree bit for bit on the poses."""
    import threading
    import types

    from ba_amd import sharding
    po = oracle_lib
    monkeypatch.setenv("BA_HIP_KOUT", "2")
    lm_dim, P = 1, 80
    sc = scene.make_scene(P, 400, 6, lm_dim=lm_dim, seed=79)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    nsel = sc.obs_per_landmark + 1
    L = sc.num_landmarks
    shards = sharding.landmark_shards(np.full(L, sc.obs_per_landmark), nranks)

    def sub(lo, hi):
        m = (sc.obs_lm >= lo) & (sc.obs_lm < hi)
        s = types.SimpleNamespace(**vars(sc))
        s.landmarks, s.lm_ref_pose = sc.landmarks[lo:hi], sc.lm_ref_pose[lo:hi]
        s.obs_z, s.obs_pose, s.obs_lm = sc.obs_z[m], sc.obs_pose[m], sc.obs_lm[m] - lo
        s.num_landmarks = hi - lo
        return s

    def make(cls, opts, s, pose_pose):
        b = cls(lm_dim, 15)
        b.Init(opts)
        b.SetGravity(sc.gravity)
        fill(b, s)
        if pose_pose:
            _add_all_residual_kinds(b, sc, po, P, unary_every=8)
        return b

    o = make(po.OracleBundleAdjuster, gn_options(po, use_dogleg=1), sc, True)
    ranks = [make(adjuster.BundleAdjuster, hip_options(use_dogleg=1, write_reduced_camera_matrix=0), sub(*shards[r]), r == 0)
             for r in range(nranks)]
    ar = sharding.ThreadAllReduce(nranks)
    for r in range(nranks):
        ranks[r].set_allreduce(ar.hook(r), r, nranks)
        ranks[r].set_collectives(ar.collectives(r))
    names = ("proj_error", "inertial_error", "unary_error", "binary_error", "pre_solve_norm", "post_solve_norm",
             "trust_region_size", "delta_norm")
    res = {}

    def run(r):
        try:
            rows = []
            for _ in range(3):
                ranks[r].Solve(1)
                s = ranks[r].summary()
                rows.append((s.result,) + tuple(getattr(s, n) for n in names) + (ranks[r].solve_is_distributed(),))
            res[r] = rows
        except Exception as exc:  # surfaced below
            res[r] = exc

    th = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not ar.failed
    for r in range(nranks):
        assert not isinstance(res[r], Exception), res[r]
    for it in range(3):
        o.Solve(1)
        so = o.summary()
        for r in range(nranks):
            row = res[r][it]
            assert row[0] == so.result and row[-1] is True
            for n, v in zip(names, row[1:-1]):
                a = getattr(so, n)
                tol = 1e-5 if n == "delta_norm" else 1e-6
                assert abs(a - v) <= tol * max(abs(a), 1e-9), (it, r, n, a, v)
    p0 = ranks[0].poses()
    for r in range(nranks):
        pr = ranks[r].poses()
        for a, b in zip(pr, p0):
            assert np.array_equal(a, b)                      # pose, velocity, bias states: bit for bit across ranks
        for a, b in zip(pr, o.poses()):
            assert rel_err(a, b) < 1e-6
    lms = np.concatenate([ranks[r].landmarks() for r in range(nranks)])
    assert rel_err(lms, o.landmarks()) < 1e-6


def _add_all_residual_kinds(b, sc, po_math, P, rng_seed=4, unary_every=10):
    """projection (already filled) + IMU between neighbours + unary prior on every k-th pose +
    binary odometry between neighbours: the shape of BASELINE.json configs[4]."""
    rng = np.random.default_rng(rng_seed)
    for i in range(P - 1):
        b.AddImuResidual(i, i + 1, sc.imu_meas[i])
    for i in range(0, P, unary_every):
        b.AddUnaryConstraint(i, sc.gt_poses[i], np.diag([1e-2] * 3 + [1e-3] * 3), True)
    for i in range(P - 1):
        t12 = po_math.se3_mul(po_math.se3_inv(sc.gt_poses[i]), sc.gt_poses[i + 1])
        t12[:3] += 0.01 * rng.normal(size=3)
        b.AddBinaryConstraint(i, i + 1, t12)


@pytest.mark.gpu
@pytest.mark.parametrize("lm_dim", [1, 3])
def test_config4_miniature_matches_oracle(oracle_lib, lm_dim):
    """BASELINE.json configs[4] in miniature: ONE problem with all four residual kinds —
    reprojection + unary priors + binary odometry + IMU pre-integration — PoseSize 15, dogleg
    trust region (BundleAdjuster.cpp:298-663, 850-1083).  S and rhs at the first linearisation,
    then errors, trust region and state over three iterations, against the oracle."""
    po = oracle_lib
    P = 40
    sc = scene.make_scene(P, 160, 6, lm_dim=lm_dim, seed=77)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, use_dogleg=1)),
                      (adjuster.BundleAdjuster, hip_options(use_dogleg=1))):
        b = cls(lm_dim, 15)
        b.Init(opts)
        b.SetGravity(sc.gravity)
        fill(b, sc)
        _add_all_residual_kinds(b, sc, po, P, unary_every=8)
        objs.append(b)
    o, h = objs
    for it in range(3):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        if it == 0:
            assert rel_err(h.S(), o.S()) < 1e-9
            assert rel_err(h.rhs(), o.rhs()) < 1e-9
        for name in ("proj_error", "inertial_error", "unary_error", "binary_error", "pre_solve_norm",
                     "post_solve_norm"):
            a, b_ = getattr(so, name), getattr(sh, name)
            assert abs(a - b_) <= 1e-6 * max(abs(a), 1e-9), (it, name, a, b_)
        assert abs(so.trust_region_size - sh.trust_region_size) <= 1e-6 * abs(so.trust_region_size)
        assert abs(so.delta_norm - sh.delta_norm) <= 1e-5 * max(so.delta_norm, 1e-12)
    _state_close(o, h, 1e-6)
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-6


_BENCH_SCENES = {}


def _bench_scene(P, L, K):
    """The bench scene of that size, generated once per test session (30 s at configs[3]); read-only."""
    if (P, L, K) not in _BENCH_SCENES:
        _BENCH_SCENES.clear()  # one at a time: the 10M-residual scene holds about a gigabyte
        _BENCH_SCENES[(P, L, K)] = scene.make_scene(P, L, K, lm_dim=1, seed=2)
    return _BENCH_SCENES[(P, L, K)]


def _bench_scene_engine(P, L, K, keep_s=False, calibrate=None):
    sc = _bench_scene(P, L, K)
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::K + 1] = False
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    eng = hipapi.Engine(1, 6)
    if calibrate:
        eng.set_calibration(4 if calibrate == "intrinsics" else 0, calibrate == "tvs")
        pa[::10] = 0  # the calibration unknowns need more than the two anchors to be observable
        if calibrate == "intrinsics":
            eng.set_landmark_ref_pixels(sc.obs_z[::K + 1])
    if keep_s:
        o = hipapi.Options()
        o.projection_outlier_threshold = 1.0
        o.use_robust_norm_for_proj_residuals = 1
        o.use_triangular_matrices = 1
        o.keep_reduced_system = 1
        eng.set_options(o)
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    return sc, eng


@pytest.mark.gpu
def test_config3_full_size_properties():
    """BASELINE.json configs[3] — the scene the metric is quoted on (10k poses / 1M landmarks /
    10M residuals, n = 59 988; bench.py's default workload and schedule: KOUT 16, left-looking
    sub-panels of 8, k_update128).  The oracle cannot factor n = 60k, so the gate is size-independent:
    (1) S delta = rhs, formed on the device from the kept copy of S (28.8 GB — never downloaded);
    (2) the step is bitwise repeatable; (3) two Gauss-Newton steps are accepted and reduce the error."""
    sc, eng = _bench_scene_engine(10000, 1000000, 10, keep_s=True)
    assert eng.num_pose_params() == 59988
    e0 = eng.linearize()
    assert eng.solve_gn() == 0
    res, rhs = eng.check_solve()
    assert rhs > 0 and res / rhs < 1e-9, (res, rhs)
    d1, l1 = eng.get_delta_gn()
    assert np.all(np.isfinite(d1)) and np.linalg.norm(d1) > 0
    eng.linearize()                      # same state: nothing was applied
    assert eng.solve_gn() == 0
    d2, l2 = eng.get_delta_gn()
    assert np.array_equal(d1, d2) and np.array_equal(l1, l2)   # no atomics anywhere: bit for bit
    errs = [e0.proj_error]
    for _ in range(2):
        eng.compose_step(0.0, 1.0)
        pre = eng.eval_residuals()
        eng.apply_step()
        post = eng.eval_residuals()
        assert post.total() < pre.total()
        errs.append(post.total())
        eng.linearize()
        assert eng.solve_gn() == 0
    assert errs[2] < errs[1] < errs[0]
    # the first step moved the poses towards the ground truth
    t, _, _ = eng.get_poses(sc.num_poses)
    assert np.linalg.norm(t[:, :3] - sc.gt_poses[:, :3]) < np.linalg.norm(sc.poses[:, :3] - sc.gt_poses[:, :3])
    eng.end_solve()
    eng.close()


@pytest.mark.gpu
def test_config3_full_size_distributed_solve_on_two_emulated_ranks():
    """The distributed reduced solve at the size bench.py runs it (configs[3]: 938 tiles, blocks of 16 tiles, 59
    panels, k_update128 with the ownership map, 0.5 GB messages): two engines on the one GPU hold half of the
    landmarks each (threads + in-process hooks) and factorise n = 59 988 together; ONE engine on the whole scene is
    the reference (it is itself gated against the oracle at every size the oracle can follow).  The Gauss-Newton
    step must be bitwise equal on both ranks, agree with the single engine to 1e-9, and the bytes moved must be
    the bytes ba_hip_dist_plan_stats predicts for this pattern (the committed fixture of tests/test_dist_plan.py)."""
    import threading

    from ba_amd import sharding
    P, L, K = 10000, 1000000, 10
    sc, single = _bench_scene_engine(P, L, K)
    single.linearize()
    assert single.solve_gn() == 0
    d_single, _ = single.get_delta_gn()
    nzL = single.factor_tile_pattern()
    single.end_solve()
    single.close()
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::K + 1] = False
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    shards = sharding.landmark_shards(np.full(L, K), 2)

    def make(lo, hi):
        sel = keep & (sc.obs_lm >= lo) & (sc.obs_lm < hi)
        eng = hipapi.Engine(1, 6)
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks[lo:hi], sc.lm_ref_pose[lo:hi])
        eng.set_projection_residuals(sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel] - lo)
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        return eng

    engs = [make(*shards[r]) for r in range(2)]
    ar = sharding.ThreadAllReduce(2)
    for r in range(2):
        engs[r].set_allreduce(ar.hook(r), r, 2)
        engs[r].set_collectives(ar.collectives(r))
        assert engs[r].solve_is_distributed()
    out = {}

    def run(r):
        try:
            engs[r].linearize()
            rc = engs[r].solve_gn()
            out[r] = (rc, engs[r].get_delta_gn()[0])
        except Exception as exc:  # surfaced below
            out[r] = exc

    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not ar.failed
    for r in range(2):
        assert not isinstance(out[r], Exception), out[r]
        assert out[r][0] == 0
    assert np.array_equal(out[0][1], out[1][1])
    assert rel_err(out[0][1], d_single) < 1e-9
    plan = hipapi.dist_plan_stats(nzL.shape[0], nzL, 2, "auto")
    cs = [engs[r].comm_stats() for r in range(2)]
    assert sum(c["chain_bytes_recv"] for c in cs) == pytest.approx(plan["chain_recv_total"], rel=1e-12)
    assert sum(c["side_bytes_recv"] for c in cs) == pytest.approx(plan["side_recv_total"], rel=1e-12)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config3_factor_tile_pattern.npz")
    d = np.load(golden)
    assert np.array_equal(np.unpackbits(d["bits"])[:nzL.size].reshape(nzL.shape), nzL)   # the fixture IS this pattern
    for e_ in engs:
        e_.end_solve()
        e_.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tvs", "intrinsics"])
def test_config3_full_size_with_calibration_unknowns(kind):
    """The configs[3] scene (10k poses / 1M landmarks / 10M residuals) with the self-calibration
    unknowns switched on: the bordered system of n + 6 (n + 4) unknowns — 9 000 border blocks from
    k_pose_border, S_kk / rhs_k from one pass over 21M calibration rows, a dense last tile row through
    the factorisation.  Size-independent gates as for the plain scene: S delta = rhs on the device,
    a bitwise repeatable step, two accepted steps that reduce the error, a camera that moves."""
    sc, eng = _bench_scene_engine(10000, 1000000, 10, keep_s=True, calibrate=kind)
    K = 6 if kind == "tvs" else 4
    n = eng.num_pose_params()
    assert n == 9000 * 6 and eng.num_calib_params() == K
    e0 = eng.linearize()
    assert eng.solve_gn() == 0
    res, rhs = eng.check_solve()
    assert rhs > 0 and res / rhs < 1e-9, (res, rhs)
    d1, l1 = eng.get_delta_gn()
    assert d1.shape[0] == n + K and np.all(np.isfinite(d1)) and np.linalg.norm(d1[n:]) > 0
    eng.linearize()
    assert eng.solve_gn() == 0
    d2, l2 = eng.get_delta_gn()
    assert np.array_equal(d1, d2) and np.array_equal(l1, l2)
    cam_before = (eng.get_cameras(1) if kind == "tvs" else eng.get_camera_params(1)).copy()
    errs = [e0.proj_error]
    for _ in range(2):
        eng.compose_step(0.0, 1.0)
        pre = eng.eval_residuals()
        eng.apply_step()
        post = eng.eval_residuals()
        assert post.total() < pre.total()
        errs.append(post.total())
        eng.linearize()
        assert eng.solve_gn() == 0
    assert errs[2] < errs[1] < errs[0]
    cam_after = eng.get_cameras(1) if kind == "tvs" else eng.get_camera_params(1)
    assert np.linalg.norm(cam_after - cam_before) > 0
    eng.end_solve()
    eng.close()


@pytest.mark.gpu
def test_config2_full_size_visual_inertial():
    """BASELINE.json configs[2] at full size: 5k poses / 500k landmarks / 5M residuals + IMU
    pre-integration, PoseSize 15 (n = 75 000), through the C++ class.  Property gate: result codes,
    dogleg steps accepted, errors decrease, repeated Solve(1) on the warm object (no rebuild)."""
    P, L = 5000, 500000
    sc = scene.make_scene(P, L, 10, lm_dim=1, seed=3)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    h = adjuster.BundleAdjuster(1, 15)
    o = adjuster.default_options()
    o.use_dogleg = 1
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    h.Init(o)
    h.SetGravity(sc.gravity)
    fill(h, sc)
    for i in range(P - 1):
        h.AddImuResidual(i, i + 1, sc.imu_meas[i])
    tot = []
    for it in range(3):
        h.Solve(1)
        s = h.summary()
        assert adjuster.RESULT_NAMES[s.result] == "Success", adjuster.RESULT_NAMES[s.result]
        assert np.isfinite(s.proj_error) and np.isfinite(s.inertial_error) and np.isfinite(s.delta_norm)
        assert s.post_solve_norm <= s.pre_solve_norm
        tot.append(s.post_solve_norm)
    # (the Huber weights are re-estimated at every linearisation, so totals of different
    # iterations are measured with different weights: only the overall decrease is asserted)
    assert tot[2] < tot[0]
    t, v, b = h.poses()
    assert np.all(np.isfinite(t)) and np.all(np.isfinite(v)) and np.all(np.isfinite(b))


@pytest.mark.gpu
def test_config4_full_size_all_residual_kinds(oracle_lib):
    """BASELINE.json configs[4] at full size on ONE GPU: 10k poses / 1M landmarks / 10M residuals +
    IMU + unary priors on every 100th pose + binary odometry, PoseSize 15, dogleg; n = 150 000 —
    S is 180 GB of the 288 GB of HBM.  Property gate as for configs[2]."""
    P, L = 10000, 1000000
    sc = scene.make_scene(P, L, 10, lm_dim=1, seed=3)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    h = adjuster.BundleAdjuster(1, 15)
    o = adjuster.default_options()
    o.use_dogleg = 1
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    h.Init(o)
    h.SetGravity(sc.gravity)
    fill(h, sc)
    _add_all_residual_kinds(h, sc, oracle_lib, P, unary_every=100)
    tot = []
    for it in range(2):
        h.Solve(1)
        s = h.summary()
        assert adjuster.RESULT_NAMES[s.result] == "Success", adjuster.RESULT_NAMES[s.result]
        for name in ("proj_error", "inertial_error", "unary_error", "binary_error", "delta_norm"):
            assert np.isfinite(getattr(s, name)), name
        assert s.post_solve_norm <= s.pre_solve_norm
        tot.append(s.post_solve_norm)
    assert tot[1] < tot[0]
    t, v, b = h.poses()
    assert np.all(np.isfinite(t)) and np.all(np.isfinite(v)) and np.all(np.isfinite(b))


# ---- multi-rank paths: native RCCL, class-level sharding ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("keep_s,one_comm", [(0, 0), (1, 0), (0, 1)],
                         ids=["distributed_solve", "replicated_solve", "distributed_one_communicator"])
def test_native_rccl_communicator_single_rank(oracle_lib, monkeypatch, keep_s, one_comm):
    """ba_hip_comm_init: the engine loads librccl itself and runs the cross-shard sums and the
    collectives of the distributed reduced solve on its own ncclComm.  One rank (all this box has):
    the sharded code paths are forced on, every all-reduce / reduce-scatter / broadcast goes through
    RCCL, and the results must equal the plain single engine and the oracle."""
    lm_dim = 1
    if one_comm:   # no ncclCommSplit duplicate: the side transfers are ordered into the chain stream
        monkeypatch.setenv("BA_HIP_ONE_COMM", "1")
    sc = scene.make_scene(300, 3000, 6, lm_dim=lm_dim, seed=67)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::sc.obs_per_landmark + 1] = False

    def make(native):
        eng = hipapi.Engine(lm_dim, 6)
        o = hipapi.Options()
        o.projection_outlier_threshold = 1.0
        o.use_robust_norm_for_proj_residuals = 1
        o.use_triangular_matrices = 1
        o.keep_reduced_system = keep_s   # the distributed solve is off while S must stay readable
        eng.set_options(o)
        if native:
            eng.comm_init(hipapi.Engine.comm_unique_id(), 0, 1)
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
        eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        return eng

    plain, native = make(False), make(True)
    assert native.solve_is_distributed() == (keep_s == 0) and not plain.solve_is_distributed()
    out = {}
    _run_engine_steps(plain, 3, out, "plain")
    _run_engine_steps(native, 3, out, "native")
    for k in ("plain", "native"):
        assert not isinstance(out[k], Exception), out[k]
    for a, b in zip(out["plain"], out["native"]):
        assert a[0] == b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            assert abs(x - y) <= 1e-9 * max(abs(x), 1e-12)
    pp, _, _ = plain.get_poses(sc.num_poses)
    pn, _, _ = native.get_poses(sc.num_poses)
    assert rel_err(pn, pp) < 1e-9
    ref = _oracle_gn_run(oracle_lib, sc, lm_dim, pa, 3)
    _check_against_oracle(ref, out, "native", pn)
    cs = native.comm_stats()
    if keep_s == 0:
        # one rank: the rows travel to the rank itself — through ncclSend / ncclRecv on BOTH communicators
        # (chain: square broadcasts + urgent rows; side: ncclCommSplit duplicate, the rest of every panel)
        assert cs["factorisations"] == 3 and cs["chain_messages"] > 0 and cs["side_messages"] > 0
        assert cs["chain_bytes_sent"] > 0 and cs["side_bytes_sent"] > 0 and cs["side_bytes_recv"] == cs["side_bytes_sent"]
        assert cs["reduce_scatter_bytes"] > 0
    assert cs["allreduce_bytes"] > 0
    native.comm_destroy()
    assert not native.solve_is_distributed()
    for e_ in (plain, native):
        e_.end_solve()
        e_.close()


@pytest.mark.gpu
@pytest.mark.parametrize("distributed", [1, 0], ids=["distributed_solve", "replicated_solve"])
def test_class_level_native_communicator_single_rank(oracle_lib, distributed):
    """ba::BundleAdjuster::SetCommunicator (round 3): the C++ class joins the engine-owned RCCL communicator by
    itself — no hook, no poking the engine — and switches between the distributed and the replicated reduced
    solve.  One rank (all this box has): every collective and both communicators run through RCCL; three
    Solve(1) calls must agree with a plain adjuster and with the oracle (visual + unary priors, 300 poses)."""
    po = oracle_lib
    lm_dim = 1
    sc = scene.make_scene(300, 3000, 6, lm_dim=lm_dim, seed=67)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0

    def make(cls, opts):
        b = cls(lm_dim, 6)
        b.Init(opts)
        fill(b, sc, active=pa)
        for i in range(0, sc.num_poses, 25):
            b.AddUnaryConstraint(i, sc.gt_poses[i], np.diag([1e-2] * 3 + [1e-3] * 3), True)
        return b

    o = make(po.OracleBundleAdjuster, gn_options(po))
    plain = make(adjuster.BundleAdjuster, hip_options(write_reduced_camera_matrix=0))
    native = make(adjuster.BundleAdjuster, hip_options(write_reduced_camera_matrix=0))
    native.set_communicator(hipapi.Engine.comm_unique_id(), 0, 1, distributed_solve=bool(distributed))
    for it in range(3):
        o.Solve(1); plain.Solve(1); native.Solve(1)
        so, sp, sn = o.summary(), plain.summary(), native.summary()
        assert so.result == sp.result == sn.result
        assert native.solve_is_distributed() == bool(distributed) and not plain.solve_is_distributed()
        for a, b in ((sn.proj_error, sp.proj_error), (sn.unary_error, sp.unary_error), (sn.delta_norm, sp.delta_norm)):
            assert abs(a - b) <= 1e-9 * max(abs(b), 1e-12)
        assert abs(sn.proj_error - so.proj_error) <= 1e-8 * so.proj_error
        if it == 0:
            assert rel_err(native.delta_p(), o.delta_p()) < 1e-8      # north_star: 1e-6 on delta_x
    assert rel_err(native.poses()[0], plain.poses()[0]) < 1e-9
    assert rel_err(native.poses()[0], o.poses()[0]) < 1e-8
    assert rel_err(native.landmarks(), o.landmarks()) < 1e-8
    cs = native.engine().comm_stats()
    assert cs["allreduce_bytes"] > 0
    if distributed:
        assert cs["factorisations"] == 3 and cs["chain_messages"] > 0 and cs["side_messages"] > 0
    else:
        assert cs["factorisations"] == 0
    native.set_communicator(None, 0, 1)   # ClearCommunicator: back to a plain single engine
    native.Solve(1); plain.Solve(1)
    assert not native.solve_is_distributed()
    assert rel_err(native.poses()[0], plain.poses()[0]) < 1e-9


@pytest.mark.gpu
def test_class_level_sharding_uses_global_counts_for_the_gauge_masks(oracle_lib):
    """Two landmark shards driven through the C++ class (SetAllReduce), unary priors on rank 0 only
    and one pose that only shard 0 observes: the gauge masks (BundleAdjuster.cpp:1237-1330) must
    come from GLOBAL residual counts — with rank-local counts shard 1 would regularise the root
    pose and fully mask the pose it does not see (round-1 advisor finding).  Reference: one
    adjuster holding everything, and the oracle."""
    import threading
    import types

    from ba_amd import sharding
    po = oracle_lib
    lm_dim = 1
    sc = scene.make_scene(40, 200, 6, lm_dim=lm_dim, seed=91)
    nsel = sc.obs_per_landmark + 1
    L = sc.num_landmarks
    half = L // 2
    lonely = int(sc.obs_pose[nsel * 3 + 2])           # a pose that landmark 3 (shard 0) observes
    idx = np.arange(len(sc.obs_pose))
    drop = (sc.obs_lm >= half) & (sc.obs_pose == lonely) & (idx % nsel != 0)
    drop |= (sc.lm_ref_pose[sc.obs_lm] == lonely) & (sc.obs_lm >= half)   # nor as a reference pose there
    keep = ~drop

    def sub(lo, hi):
        m = keep & (sc.obs_lm >= lo) & (sc.obs_lm < hi)
        s = types.SimpleNamespace(**vars(sc))
        s.landmarks, s.lm_ref_pose = sc.landmarks[lo:hi], sc.lm_ref_pose[lo:hi]
        s.obs_z, s.obs_pose, s.obs_lm = sc.obs_z[m], sc.obs_pose[m], sc.obs_lm[m] - lo
        s.num_landmarks = hi - lo
        return s

    def priors(b):
        for i in range(0, sc.num_poses, 8):
            b.AddUnaryConstraint(i, sc.gt_poses[i], np.diag([1e-2] * 3 + [1e-3] * 3), True)

    def make(cls, opts, s, with_priors):
        b = cls(lm_dim, 6)
        b.Init(opts)
        fill(b, s)
        if with_priors:
            priors(b)
        return b

    whole = sub(0, L)
    assert not np.any((whole.obs_pose == lonely) & (whole.obs_lm >= half))
    o = make(po.OracleBundleAdjuster, gn_options(po), whole, True)
    single = make(adjuster.BundleAdjuster, hip_options(write_reduced_camera_matrix=0), whole, True)
    ranks = [make(adjuster.BundleAdjuster, hip_options(write_reduced_camera_matrix=0), sub(0, half), True),
             make(adjuster.BundleAdjuster, hip_options(write_reduced_camera_matrix=0), sub(half, L), False)]
    ar = sharding.ThreadAllReduce(2)
    for r in range(2):
        ranks[r].set_allreduce(ar.hook(r), r, 2)
    res = {}

    def run(r):
        try:
            rows = []
            for _ in range(3):
                ranks[r].Solve(1)
                s = ranks[r].summary()
                rows.append((s.result, s.proj_error, s.unary_error, s.delta_norm))
            res[r] = rows
        except Exception as exc:
            res[r] = exc

    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    rows_single, rows_o = [], []
    for _ in range(3):
        single.Solve(1)
        o.Solve(1)
        s, so = single.summary(), o.summary()
        rows_single.append((s.result, s.proj_error, s.unary_error, s.delta_norm))
        rows_o.append((so.result, so.proj_error, so.unary_error, so.delta_norm))
    for t in th:
        t.join(timeout=180)
    assert not ar.failed
    for r in range(2):
        assert not isinstance(res[r], Exception), res[r]
    for it in range(3):
        assert res[0][it] == res[1][it] or np.allclose(res[0][it], res[1][it], rtol=1e-12)  # same sums on both ranks
        for a, b_ in zip(res[0][it], rows_single[it]):
            assert abs(a - b_) <= 1e-8 * max(abs(b_), 1e-12)
        for a, b_ in zip(res[0][it], rows_o[it]):
            assert abs(a - b_) <= 1e-7 * max(abs(b_), 1e-12)
    ps, po_ = single.poses()[0], o.poses()[0]
    p0, p1 = ranks[0].poses()[0], ranks[1].poses()[0]
    assert np.array_equal(p0, p1)
    assert rel_err(p0, ps) < 1e-9 and rel_err(p0, po_) < 1e-8


@pytest.mark.gpu
def test_rank_deficiency_guard_reports_factorization_error(oracle_lib):
    """Options::factorization_pivot_tolerance (extension, ba_hip_options::pivot_rel_tolerance).
    A pose seen through ONE world-point observation has a rank-2 block: S is singular.  The reference
    reports FactorizationError only when an elimination cancels to EXACTLY zero (Eigen info(),
    BundleAdjuster.cpp:756-759) — rounding-order luck, so engine and oracle may both let an arbitrary
    step through (round-1 soak: "oracle 4, engine 0" on six such scenes).  With the guard on, the
    engine reports the failure deterministically; on a well-posed scene the guard changes nothing."""
    import types
    po = oracle_lib
    sc = scene.make_scene(30, 120, 6, lm_dim=3, seed=5)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    lonely = int(np.setdiff1d(np.arange(sc.num_poses), sc.anchor_poses)[7])
    idx = np.nonzero(sc.obs_pose == lonely)[0]
    assert len(idx) > 3
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[idx[1:]] = False                      # the pose keeps a single observation
    s1 = types.SimpleNamespace(**vars(sc))
    s1.obs_z, s1.obs_pose, s1.obs_lm = sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep]

    def solve(scn, tol):
        h = adjuster.BundleAdjuster(3, 6)
        h.Init(hip_options(factorization_pivot_tolerance=tol))
        fill(h, scn, active=pa)
        h.Solve(1)
        return h
    # singular: reported with the guard (whatever the unguarded rounding does)
    h = solve(s1, 1e-10)
    assert adjuster.RESULT_NAMES[h.summary().result] == "FactorizationError"
    th, _, _ = h.poses()
    assert rel_err(th, sc.poses) < 1e-15       # nothing was applied
    free = adjuster.RESULT_NAMES[solve(s1, 0.0).summary().result]
    assert free in ("Success", "ErrorIncreased", "FactorizationError")   # reference semantics: luck
    # well-posed: the guard is inert — same result code, bitwise the same step
    a, b = solve(sc, 0.0), solve(sc, 1e-10)
    assert adjuster.RESULT_NAMES[a.summary().result] == adjuster.RESULT_NAMES[b.summary().result] == "Success"
    assert np.array_equal(a.delta_p(), b.delta_p())
    o = po.OracleBundleAdjuster(3, 6)
    o.Init(gn_options(po))
    fill(o, sc, active=pa)
    o.Solve(1)
    assert rel_err(b.delta_p(), o.delta_p()) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("lm_dim", [1, 3])
def test_structure_built_on_device_equals_host_build(lm_dim):
    """ba_hip_finalize builds the static lists on the GPU (structure_dev.hip: radix sorts, scans,
    generation kernels that mirror the host loops); the host builder (structure.h — checked on the
    CPU against a dense Schur complement, tests/test_structure_lists.py) is the specification.  Same
    scene through both: identical list sizes and, because every list has the same order, a bitwise
    identical S, rhs and Gauss-Newton step.  Includes inactive poses / landmarks, duplicate
    observations, observations from the reference pose and a landmark with more than 64 observations."""
    sc = scene.make_scene(60, 300, 7, lm_dim=lm_dim, seed=123)
    nsel = sc.obs_per_landmark + (1 if lm_dim == 1 else 0)
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    if lm_dim == 1:
        keep[::nsel] = False
    z, pose, lm = sc.obs_z[keep].copy(), sc.obs_pose[keep].copy(), sc.obs_lm[keep].copy()
    rng = np.random.default_rng(4)
    # duplicates, reference-pose observations (second camera semantics), a 150-observation landmark
    dup = rng.choice(len(pose), 40, replace=False)
    z, pose, lm = np.concatenate([z, z[dup] + 0.3]), np.concatenate([pose, pose[dup]]), np.concatenate([lm, lm[dup]])
    big = rng.integers(0, sc.num_poses, 150).astype(pose.dtype)
    zb = sc.obs_z[keep][:150] + rng.normal(0, 1.0, (150, 2))
    z, pose, lm = np.concatenate([z, zb]), np.concatenate([pose, big]), np.concatenate([lm, np.full(150, 7, dtype=lm.dtype)])
    perm = rng.permutation(len(pose))
    z, pose, lm = z[perm], pose[perm], lm[perm]
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[[0, 9, 31]] = 0
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    la[[2, 50, 51]] = 0

    def run(host):
        eng = hipapi.Engine(lm_dim, 6)
        o = hipapi.Options()
        o.projection_outlier_threshold = 1.0
        o.use_robust_norm_for_proj_residuals = 1
        o.use_triangular_matrices = 1
        o.keep_reduced_system = 1
        eng.set_options(o)
        eng.debug_set(5, 1 if host else 0)
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks, sc.lm_ref_pose, is_active=la)
        eng.set_projection_residuals(z, pose, lm)
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        e0 = eng.linearize()
        S, (rhs, rhs_p, rhs_l) = eng.get_S(), eng.get_rhs()
        rc = eng.solve_gn()
        dp, dl = eng.get_delta_gn()
        w = eng.get_proj_weights(len(pose))
        st = eng.structure_stats()
        eng.close()
        return e0.proj_error, S, rhs, rhs_p, rhs_l, rc, dp, dl, w, st
    h, d = run(True), run(False)
    for k in ("observations", "incidences", "factor_rows", "pair_blocks", "pair_entries", "tile_refs", "pose_entries",
              "linearize_waves", "tiles_S", "tiles_L"):
        assert h[9][k] == d[9][k], k
    assert h[0] == d[0] and h[5] == d[5]
    for a, b in zip(h[1:5], d[1:5]):
        assert np.array_equal(a, b)
    assert np.array_equal(h[6], d[6]) and np.array_equal(h[7], d[7]) and np.array_equal(h[8], d[8])


# ---- camera-extrinsics calibration (DoTvs instantiations) --------------------------
T_VS_MOUNT = np.concatenate([[0.05, -0.02, 0.1], scene.quat_exp(np.array([0.02, -0.03, 0.01]))])


def _calib_scene(P=40, L=160, K=8, seed=2, fixed_every=3, perturb=(0.06, -0.05, 0.05, 0.02, -0.03, 0.02), po=None,
                 **kw):
    """A banked trajectory with the camera mounted at T_VS_MOUNT, every `fixed_every`-th vehicle
    pose held at ground truth (T_vs observable), landmarks handed over for a wrong mount guess."""
    sc = scene.mount_camera(scene.make_scene(P, L, K, lm_dim=1, seed=seed, roll_amp=0.6, **kw), T_VS_MOUNT)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[::fixed_every] = 0
    sc.poses[::fixed_every] = sc.gt_poses[::fixed_every]
    t0 = po.exp_decoupled(T_VS_MOUNT, np.asarray(perturb, dtype=np.float64))
    sc.landmarks = scene.remount_landmarks(sc, T_VS_MOUNT, t0)
    return sc, pa, t0


def _calib_pair(po, sc, pa, t0, pose_dim=6, imu=False, **kw):
    o = po.OracleBundleAdjuster(1, pose_dim, do_tvs=True)
    o.Init(gn_options(po, **kw))
    h = adjuster.BundleAdjuster(1, pose_dim, do_tvs=True)
    h.Init(hip_options(**kw))
    for b in (o, h):
        if imu:
            b.SetGravity(sc.gravity)
        b.AddCamera(sc.cam_params, t0)
        b.add_poses(sc.poses, v_w=getattr(sc, "init_vel", None), b=getattr(sc, "init_bias", None), is_active=pa,
                    time=getattr(sc, "pose_time", None))
        b.add_landmarks(sc.landmarks, sc.lm_ref_pose)
        b.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
        if imu:
            for i in range(sc.num_poses - 1):
                b.AddImuResidual(i, i + 1, sc.imu_meas[i])
    return o, h


@pytest.mark.gpu
@pytest.mark.parametrize("triangular", [1, 0])
def test_calibration_reduced_system_and_step(oracle_lib, triangular):
    """The bordered (n + 6) system of BundleAdjuster.cpp:493-583 — dz_dtvs per residual, S_pk, S_kk,
    rhs_k before and after the Schur complement — and the Gauss-Newton step [delta_p ; delta_k],
    delta_l against the oracle."""
    po = oracle_lib
    sc, pa, t0 = _calib_scene(P=30, L=90, K=6, seed=7, po=po)
    o, h = _calib_pair(po, sc, pa, t0, apply_results=0, use_triangular_matrices=triangular)
    o.Solve(1)
    h.Solve(1)
    n = o.num_pose_params()
    assert h.num_pose_params() == n and h.engine().num_calib_params() == 6
    w = np.sqrt(o.proj_weights())[:, None, None]
    assert rel_err(h.proj_tvs_jacobians(), w * o.proj_tvs_jacobians()) < 1e-11
    So, Sh = o.S(), h.S()
    assert Sh.shape == (n + 6, n + 6)
    assert rel_err(Sh[:n, :n], So[:n, :n]) < 1e-12
    assert rel_err(Sh[:n, n:], So[:n, n:]) < 1e-11 and np.abs(So[:n, n:]).max() > 1
    assert rel_err(Sh[n:, n:], So[n:, n:]) < 1e-11
    assert rel_err(Sh[n:, :n], So[n:, :n]) < 1e-11 if not triangular else np.all(Sh[n:, :n] == 0)
    assert rel_err(h.rhs(), o.rhs()) < 1e-11
    assert rel_err(h.rhs_k(), o.rhs_k()) < 1e-11
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-8
    assert rel_err(h.delta_k(), o.delta_k()) < 1e-8
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("use_dogleg", [0, 1])
def test_calibration_iterations_track_oracle_and_recover_the_mount(oracle_lib, use_dogleg):
    """Six iterations from a wrong T_vs: per-iteration summaries, the rig's camera pose, poses and
    landmarks follow the oracle, and T_vs ends close to the mount the scene was rendered with."""
    po = oracle_lib
    sc, pa, t0 = _calib_scene(po=po, outlier_frac=0.0, pixel_sigma=0.3)
    o, h = _calib_pair(po, sc, pa, t0, use_dogleg=use_dogleg)
    err0 = np.linalg.norm(po.log_decoupled(t0, T_VS_MOUNT))
    for it in range(6):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result, it
        assert abs(so.proj_error - sh.proj_error) < 1e-7 * so.proj_error, it
        assert abs(so.delta_norm - sh.delta_norm) < 1e-6 * max(so.delta_norm, 1e-12), it
        if use_dogleg:
            assert abs(so.trust_region_size - sh.trust_region_size) <= 1e-7 * abs(so.trust_region_size)
        assert rel_err(h.camera_pose(0), o.camera_pose(0)) < 1e-8, it
    to, _, _ = o.poses()
    th, _, _ = h.poses()
    assert rel_err(th, to) < 1e-7
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-7
    err = np.linalg.norm(po.log_decoupled(h.camera_pose(0), T_VS_MOUNT))
    assert err < 0.2 * err0, (err0, err)


@pytest.mark.gpu
def test_calibration_multi_iteration_solve_and_rejected_step(oracle_lib):
    """Solve(4) in one call equals the oracle's; then an overshooting step (gn_damping 40) is rejected:
    poses and landmarks are restored, T_vs keeps the rejected update exactly as in the reference
    (BundleAdjuster.cpp:72-83 is outside the copies restored at :1139-1149)."""
    po = oracle_lib
    sc, pa, t0 = _calib_scene(P=30, L=90, K=6, seed=11, po=po)
    o, h = _calib_pair(po, sc, pa, t0)
    o.Solve(4)
    h.Solve(4)
    assert o.summary().iterations_run == h.summary().iterations_run
    assert rel_err(h.camera_pose(0), o.camera_pose(0)) < 1e-8
    before_o, before_h = o.camera_pose(0).copy(), h.camera_pose(0).copy()
    po_before, _, _ = h.poses()
    o.Solve(1, 40.0)
    h.Solve(1, 40.0)
    assert adjuster.RESULT_NAMES[h.summary().result] == "ErrorIncreased"
    assert o.summary().result == h.summary().result
    po_after, _, _ = h.poses()
    assert rel_err(po_after, po_before) < 1e-12                        # poses restored
    assert np.linalg.norm(o.camera_pose(0) - before_o) > 1e-6           # the oracle's T_vs moved ...
    assert rel_err(h.camera_pose(0) - before_h, o.camera_pose(0) - before_o) < 1e-5  # ... and so did ours, alike
    # the world points written back at the end of that Solve() come from the restored caches (the
    # T_vs BEFORE the rejected step) on both sides
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-10
    # a LINEARISATION in that state — the next Solve() calls — mixes cached T_sw (old T_vs) and the rig
    # (new T_vs) inside the reference's Jacobian chains: the engine switches to the chain variant of
    # the linearisation kernel (dmath.h proj_chain_two_tvs) until an applied step rebuilds the caches
    for _ in range(3):
        o.Solve(1)
        h.Solve(1)
        assert o.summary().result == h.summary().result
        assert abs(o.summary().proj_error - h.summary().proj_error) < 1e-7 * o.summary().proj_error
        assert rel_err(h.camera_pose(0), o.camera_pose(0)) < 1e-7
    assert rel_err(h.poses()[0], o.poses()[0]) < 1e-7
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-7


@pytest.mark.gpu
def test_calibration_with_inertial_residuals(oracle_lib):
    """<1, 15, 0, true> — the reference's visual-inertial self-calibration instantiation
    (BundleAdjuster.cpp:1816-1822 with CalibSize 0): the border couples to 15-wide pose blocks."""
    po = oracle_lib
    P = 30
    sc = scene.make_scene(P, 90, 6, lm_dim=1, seed=5)
    scene.add_inertial(sc, period=60.0 * P / 100.0)  # the IMU of the synthetic scene sits in the camera frame:
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])        # the true mount is the identity
    pa = np.ones(P, dtype=np.uint8)
    pa[0] = 0
    t0 = po.exp_decoupled(ident, np.array([0.02, -0.02, 0.02, 0.01, -0.01, 0.01]))
    sc.landmarks = scene.remount_landmarks(sc, ident, t0)
    o, h = _calib_pair(po, sc, pa, t0, pose_dim=15, imu=True)
    for it in range(3):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        assert abs(so.proj_error - sh.proj_error) < 1e-6 * so.proj_error
        assert abs(so.inertial_error - sh.inertial_error) < 1e-6 * max(so.inertial_error, 1e-9)
        assert rel_err(h.camera_pose(0), o.camera_pose(0)) < 1e-7
    to, vo, bo = o.poses()
    th, vh, bh = h.poses()
    assert rel_err(th, to) < 1e-6 and rel_err(vh, vo) < 1e-5


@pytest.mark.gpu
def test_calibration_engine_refuses_what_it_does_not_implement():
    eng = hipapi.Engine(3, 6)
    with pytest.raises(hipapi.HipError):
        eng.set_calibration(0, True)      # dz_dtvs exists for LmSize 1 only
    eng.close()
    with pytest.raises(ValueError):
        adjuster.BundleAdjuster(3, 6, do_tvs=True)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [30, 32], ids=["one_tile", "straddling_tiles"])
def test_calibration_marginals(oracle_lib, P):
    """Options::calculate_calibration_marginals (BundleAdjuster.cpp:771-784): the T_vs block of S^-1,
    read from the factor (no extra solves) — against the oracle's six unit-vector solves and a dense
    inverse.  P = 32 with every third pose fixed: 21 active poses, n = 126 = 64 + 62, the six
    calibration rows straddle a tile boundary of the factor."""
    po = oracle_lib
    sc, pa, t0 = _calib_scene(P=P, L=90, K=6, seed=7, po=po)
    o, h = _calib_pair(po, sc, pa, t0, apply_results=0, use_triangular_matrices=0, calculate_calibration_marginals=1)
    o.Solve(1)
    h.Solve(1)
    n = o.num_pose_params()
    if P == 32:
        assert n % 64 > 58
    cov_h, cov_o = h.calibration_marginals(), o.calibration_marginals()
    assert cov_h.shape == (6, 6)
    assert rel_err(cov_h, cov_o) < 1e-7
    assert rel_err(cov_h, np.linalg.inv(o.S())[n:, n:]) < 1e-6
    assert np.all(np.linalg.eigvalsh(0.5 * (cov_h + cov_h.T)) > 0)


# ---- camera-intrinsics calibration (CalibSize = 4: fx, fy, u0, v0 of the pinhole model; CalibSize = 5:
# fx, fy, u0, v0, w of a FOV camera — the reference's SelfCalBundleAdjuster) -----------------------------
FOV_W = 0.93
CAMERA_MODELS = pytest.mark.parametrize("fov", [False, True], ids=["pinhole", "fov_camera"])


def _intrinsics_pair(po, sc, pa, wrong, pose_dim=6, **kw):
    o = po.OracleBundleAdjuster(1, pose_dim, calib_size=len(wrong))
    o.Init(gn_options(po, **kw))
    h = adjuster.BundleAdjuster(1, pose_dim, calib_size=len(wrong))
    h.Init(hip_options(**kw))
    for b in (o, h):
        b.AddCamera(wrong)
        b.add_poses(sc.poses, is_active=pa)
        b.add_landmarks(sc.landmarks, sc.lm_ref_pose)
        b.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
    return o, h


def _intrinsics_scene(P=40, L=160, K=8, seed=2, fov=False, **kw):
    sc = scene.make_scene(P, L, K, lm_dim=1, seed=seed, roll_amp=0.6, **kw)
    if fov:
        scene.to_fov_camera(sc, FOV_W)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[::3] = 0
    sc.poses[::3] = sc.gt_poses[::3]
    return sc, pa, np.asarray(sc.cam_params) * np.array([1.03, 0.97, 1.02, 0.98, 1.04][:len(sc.cam_params)])


@pytest.mark.gpu
@CAMERA_MODELS
@pytest.mark.parametrize("triangular", [1, 0])
def test_intrinsics_calibration_reduced_system_and_step(oracle_lib, triangular, fov):
    """CalibSize 4 / 5: dz_dcam_params per residual, the bordered (n + K) system, the step and the
    marginals against the oracle (BundleAdjuster.cpp:493-583, 771-784; parallel_algos.h:114-118)."""
    po = oracle_lib
    sc, pa, wrong = _intrinsics_scene(P=30, L=90, K=6, seed=7, fov=fov)
    K = len(wrong)
    o, h = _intrinsics_pair(po, sc, pa, wrong, apply_results=0, use_triangular_matrices=triangular,
                            calculate_calibration_marginals=1)
    o.Solve(1)
    h.Solve(1)
    n = o.num_pose_params()
    assert h.num_pose_params() == n and h.engine().num_calib_params() == K
    w = np.sqrt(o.proj_weights())[:, None, None]
    assert rel_err(h.proj_calib_jacobians(), w * o.proj_calib_jacobians()) < 1e-11
    So, Sh = o.S(), h.S()
    assert Sh.shape == (n + K, n + K)
    assert rel_err(Sh[:n, :n], So[:n, :n]) < 1e-12
    assert rel_err(Sh[:n, n:], So[:n, n:]) < 1e-11 and np.abs(So[:n, n:]).max() > 0.1
    assert rel_err(Sh[n:, n:], So[n:, n:]) < 1e-11
    assert rel_err(h.rhs(), o.rhs()) < 1e-11
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-8
    assert rel_err(h.delta_k(), o.delta_k()) < 1e-8
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-8
    if not triangular:
        assert rel_err(h.calibration_marginals(), o.calibration_marginals()) < 1e-7


@pytest.mark.gpu
@CAMERA_MODELS
@pytest.mark.parametrize("use_dogleg", [0, 1])
def test_intrinsics_calibration_iterations_track_oracle_and_recover_the_camera(oracle_lib, use_dogleg, fov):
    """Six iterations from wrong camera parameters (pinhole: four, FOV camera: five): summaries, the rig's parameters, poses and
    landmarks (whose rays are re-derived from the reference pixels after every step) follow the oracle,
    and the parameters end close to the ones the scene was rendered with."""
    po = oracle_lib
    sc, pa, wrong = _intrinsics_scene(outlier_frac=0.0, pixel_sigma=0.3, fov=fov)
    o, h = _intrinsics_pair(po, sc, pa, wrong, use_dogleg=use_dogleg)
    err0 = np.linalg.norm(wrong - sc.cam_params)
    for it in range(6):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result, it
        assert abs(so.proj_error - sh.proj_error) < 1e-7 * so.proj_error, it
        assert abs(so.delta_norm - sh.delta_norm) < 1e-6 * max(so.delta_norm, 1e-12), it
        assert rel_err(h.camera_params(0), o.camera_params(0)) < 1e-9, it
    to, _, _ = o.poses()
    th, _, _ = h.poses()
    assert rel_err(th, to) < 1e-7
    assert rel_err(h.landmarks(), o.landmarks()) < 1e-7
    assert np.linalg.norm(h.camera_params(0) - sc.cam_params) < 0.2 * err0


@pytest.mark.gpu
@CAMERA_MODELS
def test_intrinsics_calibration_rejected_step_restores_the_parameters(oracle_lib, fov):
    """Unlike T_vs the intrinsics ARE restored when a step is rejected (params_backup,
    BundleAdjuster.cpp:1025-1028, 1066, 1099-1102, 1147)."""
    po = oracle_lib
    sc, pa, wrong = _intrinsics_scene(P=30, L=90, K=6, seed=11, fov=fov)
    o, h = _intrinsics_pair(po, sc, pa, wrong)
    o.Solve(3)
    h.Solve(3)
    assert rel_err(h.camera_params(0), o.camera_params(0)) < 1e-9
    before = h.camera_params(0).copy()
    lm_before = h.landmarks().copy()
    o.Solve(1, 40.0)
    h.Solve(1, 40.0)
    assert adjuster.RESULT_NAMES[h.summary().result] == "ErrorIncreased"
    assert o.summary().result == h.summary().result
    assert np.array_equal(h.camera_params(0), before)
    assert rel_err(h.landmarks(), lm_before) < 1e-12
    assert rel_err(o.camera_params(0), before) < 1e-9


@pytest.mark.gpu
def test_calibration_combinations_that_are_refused():
    eng = hipapi.Engine(1, 6)
    with pytest.raises(hipapi.HipError):
        eng.set_calibration(4, True)      # the reference wipes the intrinsics columns in this combination
    with pytest.raises(hipapi.HipError):
        eng.set_calibration(6, False)     # no camera model with six parameters
    eng.close()
    with pytest.raises(ValueError):
        adjuster.BundleAdjuster(1, 6, do_tvs=True, calib_size=4)
    # CalibSize must be the parameter count of camera 0 (parallel_algos.h:115-118 assigns a
    # 2 x NumParams matrix to a 2 x CalibSize block): SolverError, nothing moved
    sc = scene.make_scene(12, 30, 4, lm_dim=1, seed=1)
    for calib_size, fov in ((5, False), (4, True)):
        cam = np.append(sc.cam_params, FOV_W) if fov else np.asarray(sc.cam_params)
        h = adjuster.BundleAdjuster(1, 6, calib_size=calib_size)
        h.Init(hip_options())
        h.AddCamera(cam)
        h.add_poses(sc.poses)
        h.add_landmarks(sc.landmarks, sc.lm_ref_pose)
        h.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
        h.Solve(1)
        assert adjuster.RESULT_NAMES[h.summary().result] == "SolverError"
        assert np.array_equal(h.camera_params(0), cam)
    # per-pose intrinsics are four pinhole parameters: not offered on a rig with a FovCamera
    h = adjuster.BundleAdjuster(1, 6)
    h.Init(hip_options())
    h.AddCamera(np.append(sc.cam_params, FOV_W))
    h.add_poses(sc.poses)
    h.add_landmarks(sc.landmarks, sc.lm_ref_pose)
    h.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
    h.SetPoseCamParams(np.tile(np.asarray(sc.cam_params), (sc.num_poses, 1)))
    h.Solve(1)
    assert adjuster.RESULT_NAMES[h.summary().result] == "SolverError"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tvs", "intrinsics", "fov"])
def test_calibration_edge_cases_match_oracle(oracle_lib, kind):
    """Both calibration kinds on a graph with a landmark seen from 150 poses (the two-pass variant of
    the linearisation kernel), duplicate observations, inactive poses and landmarks, and weights:
    reduced system, border, step against the oracle."""
    po = oracle_lib
    sc = scene.make_scene(60, 200, 7, lm_dim=1, seed=123, roll_amp=0.6)
    if kind == "fov":
        scene.to_fov_camera(sc, FOV_W)
    rng = np.random.default_rng(4)
    nsel = sc.obs_per_landmark + 1
    z, pose, lm = sc.obs_z.copy(), sc.obs_pose.copy(), sc.obs_lm.copy()
    dup = rng.choice(len(pose), 40, replace=False)
    dup = dup[dup % nsel != 0]  # not the reference observations (they define z_ref)
    big_pose = rng.integers(0, sc.num_poses, 150).astype(pose.dtype)
    big_pose = big_pose[big_pose != sc.lm_ref_pose[7]]
    zb = sc.obs_z[1:1 + len(big_pose)] + rng.normal(0, 1.0, (len(big_pose), 2))
    z = np.concatenate([z, z[dup] + 0.3, zb])
    pose = np.concatenate([pose, pose[dup], big_pose])
    lm = np.concatenate([lm, lm[dup], np.full(len(big_pose), 7, dtype=lm.dtype)])
    w = rng.uniform(0.5, 2.0, len(pose))
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[::3] = 0
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    la[[2, 50, 51]] = 0
    t_vs = T_VS_MOUNT
    kw = dict(do_tvs=True) if kind == "tvs" else dict(calib_size=len(sc.cam_params))
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po, apply_results=0, use_triangular_matrices=0)),
                      (adjuster.BundleAdjuster, hip_options(apply_results=0, use_triangular_matrices=0))):
        b = cls(1, 6, **kw)
        b.Init(opts)
        b.AddCamera(sc.cam_params, t_vs)
        b.add_poses(sc.poses, is_active=pa)
        b.add_landmarks(sc.landmarks, sc.lm_ref_pose, is_active=la)
        b.add_projection_residuals(z, pose, lm, weight=w)
        b.Solve(1)
        objs.append(b)
    o, h = objs
    n, K = o.num_pose_params(), o.num_calib_params()
    assert h.engine().structure_stats()["linearize_waves"] > 0
    ws = np.sqrt(o.proj_weights())[:, None, None]
    assert rel_err(h.proj_calib_jacobians(), ws * o.proj_calib_jacobians()) < 1e-11
    # the 150 extra observations carry pixels of other landmarks: residuals of hundreds of pixels, points
    # near the image plane, Jacobians of 1e5 and more — the Schur complement cancels several digits.
    # Rounding-order tolerances (the per-residual Jacobians above agree to 1e-11); step: north_star's 1e-6
    assert rel_err(h.S(), o.S()) < 1e-9
    assert rel_err(h.S()[:n, n:], o.S()[:n, n:]) < 1e-9 and rel_err(h.S()[n:, n:], o.S()[n:, n:]) < 1e-9
    assert rel_err(h.rhs(), o.rhs()) < 1e-9
    assert rel_err(h.delta_k(), o.delta_k()) < 1e-6 and rel_err(h.delta_p(), o.delta_p()) < 1e-6
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-6
    assert K == {"tvs": 6, "intrinsics": 4, "fov": 5}[kind]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tvs", "intrinsics", "fov"])
@pytest.mark.parametrize("distributed", [0, 1], ids=["replicated_solve", "distributed_solve"])
def test_calibration_on_landmark_shards(oracle_lib, kind, distributed):
    """Calibration unknowns with the landmarks sharded over three engines (threads + in-process
    hooks, as the other shard tests): the border blocks S_pk / S_kk and rhs_k are sums over the shards
    like the rest of S; with the collectives hook the bordered system goes through the distributed
    factorisation.  Three iterations against ONE engine and against the oracle: steps, errors, the
    camera's T_vs / parameters on every rank."""
    import threading

    from ba_amd import sharding
    po = oracle_lib
    nranks = 3
    P = 150 if distributed else 40
    sc = scene.make_scene(P, 10 * P, 6, lm_dim=1, seed=67, roll_amp=0.6, outlier_frac=0.0, pixel_sigma=0.3)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[::3] = 0
    sc.poses[::3] = sc.gt_poses[::3]
    if kind == "tvs":
        sc = scene.mount_camera(sc, T_VS_MOUNT)
        t_vs0 = po.exp_decoupled(T_VS_MOUNT, np.array([0.03, -0.02, 0.02, 0.01, -0.015, 0.01]))
        sc.landmarks = scene.remount_landmarks(sc, T_VS_MOUNT, t_vs0)
        cam0 = np.asarray(sc.cam_params, dtype=np.float64)
    else:
        if kind == "fov":
            scene.to_fov_camera(sc, FOV_W)
        t_vs0 = np.array([0, 0, 0, 0, 0, 0, 1.0])
        cam0 = np.asarray(sc.cam_params) * np.array([1.02, 0.98, 1.01, 0.99, 1.03][:len(sc.cam_params)])
    nsel = sc.obs_per_landmark + 1
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::nsel] = False
    z_ref = sc.obs_z[::nsel]

    def make(lo, hi):
        sel = keep & (sc.obs_lm >= lo) & (sc.obs_lm < hi)
        eng = hipapi.Engine(1, 6)
        eng.set_calibration(0 if kind == "tvs" else len(cam0), kind == "tvs")
        eng.set_cameras(cam0, t_vs0)
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks[lo:hi], sc.lm_ref_pose[lo:hi])
        if kind != "tvs":
            eng.set_landmark_ref_pixels(z_ref[lo:hi])
        eng.set_projection_residuals(sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel] - lo)
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        return eng

    def calib_state(eng):
        if kind == "tvs":
            return eng.get_cameras(1)[0]
        p = eng.get_camera_params(1)[0]
        return np.append(p, eng.get_camera_fov(1)[0]) if kind == "fov" else p

    L = sc.num_landmarks
    single = make(0, L)
    out = {}
    _run_engine_steps(single, 3, out, "single")
    shards = sharding.landmark_shards(np.full(L, sc.obs_per_landmark), nranks)
    engs = [make(*shards[r]) for r in range(nranks)]
    ar = sharding.ThreadAllReduce(nranks)
    for r in range(nranks):
        engs[r].set_allreduce(ar.hook(r), r, nranks)
        if distributed:
            engs[r].set_collectives(ar.collectives(r))
        assert bool(engs[r].solve_is_distributed()) == bool(distributed)
    th = [threading.Thread(target=_run_engine_steps, args=(engs[r], 3, out, r)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=180)
    assert not ar.failed
    for k in ["single"] + list(range(nranks)):
        assert not isinstance(out[k], Exception), out[k]
    n = single.num_pose_params()
    for it in range(3):
        a = out["single"][it]
        for r in range(nranks):
            b = out[r][it]
            assert a[0] == b[0] == 0
            for x, y in zip(a[1:], b[1:]):
                assert abs(x - y) <= 1e-7 * max(abs(x), 1e-12)
    for r in range(nranks):
        assert rel_err(out[(r, "delta_p")], out[("single", "delta_p")]) < 1e-7   # [delta_p ; delta_k] of iteration 0
        assert rel_err(calib_state(engs[r]), calib_state(single)) < 1e-9
        assert np.array_equal(calib_state(engs[r]), calib_state(engs[0]))        # every rank moves the camera alike
    # the oracle on the whole scene
    kw = dict(do_tvs=True) if kind == "tvs" else dict(calib_size=len(cam0))
    o = po.OracleBundleAdjuster(1, 6, **kw)
    o.Init(gn_options(po))
    o.AddCamera(cam0, t_vs0)
    o.add_poses(sc.poses, is_active=pa)
    o.add_landmarks(sc.landmarks, sc.lm_ref_pose)
    o.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
    for it in range(3):
        o.Solve(1)
        if it == 0:
            assert rel_err(out[(0, "delta_p")][:n], o.delta_p()) < 1e-6
            assert rel_err(out[(0, "delta_p")][n:], o.delta_k()) < 1e-6
        if adjuster.RESULT_NAMES[o.summary().result] == "Success":
            assert abs(out[0][it][3] - o.summary().proj_error) <= 1e-7 * o.summary().proj_error
    oc = o.camera_pose(0) if kind == "tvs" else o.camera_params(0)
    assert rel_err(calib_state(engs[0]), oc) < 1e-7
    for e_ in engs + [single]:
        e_.end_solve()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tvs", "intrinsics", "fov"])
def test_calibration_at_config1_scale_matches_oracle(oracle_lib, kind):
    """The self-calibration instantiations at the size of BASELINE.json configs[1] (1k poses / 100k
    landmarks / 1M residuals, a tenth of the poses held fixed): the first Gauss-Newton step
    [delta_p ; delta_k], delta_l and the moved camera against the oracle (north_star: 1e-6)."""
    po = oracle_lib
    sc = scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[::10] = 0
    sc.poses[::10] = sc.gt_poses[::10]
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    if kind == "tvs":
        t0 = po.exp_decoupled(ident, np.array([0.02, -0.02, 0.02, 0.005, -0.01, 0.005]))
        sc.landmarks = scene.remount_landmarks(sc, ident, t0)
        cam0, kw = np.asarray(sc.cam_params, dtype=np.float64), dict(do_tvs=True)
    else:
        if kind == "fov":
            scene.to_fov_camera(sc, FOV_W)
        cam0 = np.asarray(sc.cam_params) * np.array([1.01, 0.99, 1.005, 0.995, 1.01][:len(sc.cam_params)])
        t0, kw = ident, dict(calib_size=len(cam0))
    objs = []
    for cls, opts in ((po.OracleBundleAdjuster, gn_options(po)), (adjuster.BundleAdjuster, hip_options(write_reduced_camera_matrix=0))):
        b = cls(1, 6, **kw)
        b.Init(opts)
        b.AddCamera(cam0, t0)
        b.add_poses(sc.poses, is_active=pa)
        b.add_landmarks(sc.landmarks, sc.lm_ref_pose)
        b.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
        b.Solve(1)
        objs.append(b)
    o, h = objs
    assert o.summary().result == h.summary().result == 0
    assert abs(o.summary().proj_error - h.summary().proj_error) <= 1e-9 * o.summary().proj_error
    assert rel_err(h.delta_p(), o.delta_p()) < 1e-6
    assert rel_err(h.delta_k(), o.delta_k()) < 1e-6
    assert rel_err(h.delta_l(), o.delta_l()) < 1e-6
    co = o.camera_pose(0) if kind == "tvs" else o.camera_params(0)
    ch = h.camera_pose(0) if kind == "tvs" else h.camera_params(0)
    assert rel_err(ch, co) < 1e-9
    print("calibration (%s) at config-1 scale: delta_p %.2e delta_k %.2e delta_l %.2e" %
          (kind, rel_err(h.delta_p(), o.delta_p()), rel_err(h.delta_k(), o.delta_k()), rel_err(h.delta_l(), o.delta_l())))


@pytest.mark.gpu
@pytest.mark.parametrize("pose_dim", [9, 15])
def test_inertial_linearisation_variants_agree(pose_dim):
    """k_imu's forms — single pass (step Jacobians inside, variant 2), two passes with one lane per sample /
    residual (0), a wavefront per residual (dense products dealt to the lanes through LDS) over the
    lane-per-sample step pass (1), the same over a wavefront per sample with the RK4 Jacobian chain resident
    in LDS (4: k_imu_steps_wave, what runs on windows of up to 2048 samples) — run the same operations in
    the same order (bitwise equal when compiled for the host, tests/test_hostcheck.py;
    on the device the compiler contracts multiply-adds per code shape): S, rhs and the Gauss-Newton step
    agree to a few units in the last place."""
    P = 40
    sc = scene.make_scene(P, 400, 6, lm_dim=1, seed=9)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    pa = np.ones(P, dtype=np.uint8)
    pa[0] = 0

    def run(variant):
        h = adjuster.BundleAdjuster(1, pose_dim)
        h.Init(hip_options(apply_results=0, use_robust_norm_for_inertial_residuals=1))
        scene.populate(h, sc, active=pa, imu=True)
        h.Solve(0)                      # creates the engine and uploads the graph, no iteration
        h.engine().debug_set(6, variant)
        h.Solve(1)
        return h.summary().inertial_error, h.S(), h.rhs(), h.delta_p()
    ref = run(2)
    assert np.abs(ref[1]).max() > 0 and ref[0] > 0
    for variant in (0, 1, 4):
        got = run(variant)
        assert abs(got[0] - ref[0]) <= 1e-12 * ref[0]
        assert rel_err(got[1], ref[1]) < 1e-12 and rel_err(got[2], ref[2]) < 1e-12, variant
        assert rel_err(got[3], ref[3]) < 1e-9, variant
