"""Marginal covariances by selected inversion on the MI355X (ba_hip_compute_marginals, k_selinv.hip): pose,
pose-pair, calibration and landmark blocks against dense inverses of the reduced system S (read with
keep_reduced_system) and of the full poses + landmarks system H, assembled from the engine's Jacobians.
Tolerance per block: max(1e-9, 4.5 eps cond(S)) relative."""
import numpy as np
import pytest

from ba_amd import hipapi, scene
from helpers import _add_pose_pose

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


class Setup:
    pass


def _engine(sc, lm_dim, pa, mode=hipapi.ORDER_NATURAL, tvs=False, pose_pose=False, keep=True, extra_obs=None,
            calib=0, lm_active=None, obs=None):
    """obs = (z, pose, lm): the accepted residuals as given (scenes whose observation table is not make_scene's)."""
    eng = hipapi.Engine(lm_dim, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.keep_reduced_system = int(keep)
    eng.set_options(o)
    if tvs or calib:
        eng.set_calibration(calib, tvs)
    nsel = (sc.obs_per_landmark or 0) + (1 if lm_dim == 1 else 0)
    sel = np.ones(len(sc.obs_pose), dtype=bool)
    if lm_dim == 1 and not hasattr(sc, "revisited") and obs is None:
        sel[::nsel] = False
    if hasattr(sc, "revisited") and lm_dim == 1:
        sel &= ~np.r_[True, np.diff(sc.obs_lm) != 0]
    z, pose, lm = (sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel]) if obs is None else obs
    if extra_obs is not None:
        z, pose, lm = (np.concatenate([a, b]) for a, b in zip((z, pose, lm), extra_obs))
    eng.set_cameras(sc.cam_params, [0.01, -0.02, 0.03, 0, 0, 0, 1] if tvs else [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose, is_active=lm_active)
    if calib:
        eng.set_landmark_ref_pixels(sc.obs_z[::nsel])  # the reference frame's observation of every landmark
    eng.set_projection_residuals(z, pose, lm)
    if pose_pose:
        _add_pose_pose(eng, sc, sc.num_poses)
    eng.set_pose_ordering(mode)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    s = Setup()
    s.eng, s.sc, s.pa, s.lm_dim, s.tvs = eng, sc, pa, lm_dim, tvs
    s.D, s.K = 6, (6 if tvs else calib)
    s.obs_pose, s.obs_lm = np.asarray(pose, dtype=np.int64), np.asarray(lm, dtype=np.int64)
    return s


def _solve(s, iters=1):
    """iters Gauss-Newton iterations, the last one left factorised"""
    for it in range(iters):
        s.eng.linearize()
        assert s.eng.solve_gn() == 0
        if it + 1 < iters:
            s.eng.compose_step(0.0, 1.0)
            s.eng.apply_step()


def _natural_rows(pa, D=6):
    opt = np.full(len(pa), -1, dtype=np.int64)
    opt[pa.astype(bool)] = np.arange(int(pa.sum()))
    return opt * D


def _tol(S):
    tol = max(1e-9, 4.5 * EPS * np.linalg.cond(S))
    assert tol <= 1e-8, "scene too ill-conditioned for the check: %g" % tol
    return tol


def _blk_err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _landmark_reference(s, S, ids):
    """(l, l) blocks of inv(H), H = [[S + W V^-1 W^T, W], [W^T, V]], from the engine's Jacobians."""
    eng, sc = s.eng, s.sc
    LM = s.lm_dim
    nres = len(s.obs_pose)
    jm, jr, jl, _ = eng.get_proj_jacobians(nres)
    D, K = getattr(s, "D", 6), getattr(s, "K", 6 if s.tvs else 0)
    rows = _natural_rows(s.pa, D)
    n = S.shape[0]
    np_ = int(s.pa.sum()) * D
    jk = eng.get_calib_jacobians(nres)[:, :, :K] if K else None
    out = []
    Ws, Vs = {}, {}
    for l in ids:
        W = np.zeros((n, LM))
        V = np.zeros((LM, LM))
        for r in np.nonzero(s.obs_lm == l)[0]:
            pm, rp = s.obs_pose[r], sc.lm_ref_pose[l]
            V += jl[r].T @ jl[r]
            listed = LM != 1 or pm != rp
            if listed and rows[pm] >= 0:
                W[rows[pm]:rows[pm] + 6] += jm[r].T @ jl[r]
            if LM == 1 and listed and rows[rp] >= 0:
                W[rows[rp]:rows[rp] + 6] += jr[r].T @ jl[r]
            if jk is not None:
                W[np_:np_ + K] += jk[r].T @ jl[r]
        Ws[l], Vs[l] = W, V
    # dense H over the requested landmarks (the others are eliminated exactly: their Schur terms are in S)
    m = len(ids) * LM
    Wall = np.concatenate([Ws[l] for l in ids], 1) if ids else np.zeros((n, 0))
    Vall = np.zeros((m, m))
    for q, l in enumerate(ids):
        Vall[q * LM:(q + 1) * LM, q * LM:(q + 1) * LM] = Vs[l]
    U = S + Wall @ np.linalg.solve(Vall, Wall.T) if m else S
    H = np.block([[U, Wall], [Wall.T, Vall]])
    Hi = np.linalg.inv(H)
    for q in range(len(ids)):
        out.append(Hi[n + q * LM:n + (q + 1) * LM, n + q * LM:n + (q + 1) * LM])
    return np.array(out)


def _pose_checks(s, S, tol):
    eng = s.eng
    P = s.sc.num_poses
    act = np.nonzero(s.pa)[0]
    rows = _natural_rows(s.pa)
    Si = np.linalg.inv(S)
    got = eng.pose_marginals(act)
    for q, p in enumerate(act):
        r = rows[p]
        assert _blk_err(got[q], Si[r:r + 6, r:r + 6]) <= tol, p
    # pairs of poses that share a landmark: consecutive observations of a landmark
    a, b = [], []
    for l in range(0, s.sc.num_landmarks, 7):
        ps = [p for p in s.obs_pose[s.obs_lm == l] if s.pa[p]]
        if len(ps) >= 2 and ps[0] != ps[-1]:
            a.append(ps[0])
            b.append(ps[-1])
    assert len(a) > 3
    pair = eng.pose_pair_marginals(a, b)
    for q in range(len(a)):
        ra, rb = rows[a[q]], rows[b[q]]
        assert _blk_err(pair[q], Si[ra:ra + 6, rb:rb + 6]) <= tol
    return Si


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_pose_and_pair_blocks(lm_dim):
    """Pose and pair blocks against inv(S); fixed poses, pose-pose terms (the root pose regularised by a prior),
    an active pose count that is no multiple of 64 rows."""
    sc = scene.make_scene(83, 500, 6, lm_dim=lm_dim, seed=11)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[[9, 40]] = 0
    s = _engine(sc, lm_dim, pa, pose_pose=True)
    _solve(s)
    S = s.eng.get_S()
    assert S.shape[0] % 64 != 0
    tol = _tol(S)
    _pose_checks(s, S, tol)
    st = s.eng.marginal_stats()
    nt = (S.shape[0] + 63) // 64
    assert st["tile_products"] >= nt and st["store_bytes"] == st["store_tiles"] * 64 * 64 * 8
    assert st["selinv_ms"] > 0
    s.eng.close()


def test_calibration_border_and_landmarks_with_tvs():
    """DoTvs: six calibration rows behind the poses, straddling a tile boundary.  The K x K block read from the
    store equals calibration_marginals() and inv(S); landmark blocks equal inv(H) with the calibration rows."""
    sc = scene.make_scene(44, 300, 6, lm_dim=1, seed=12)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    # 42 active poses: 252 pose rows, the calibration rows 252..257 straddle the tile boundary at 256; priors
    # and odometry keep S well conditioned with the mount free
    s = _engine(sc, 1, pa, tvs=True, pose_pose=True)
    _solve(s)
    S = s.eng.get_S()
    n = S.shape[0]
    np_ = n - 6
    assert np_ // 64 != (n - 1) // 64, "calibration rows do not straddle a tile"
    tol = _tol(S)
    Si = np.linalg.inv(S)
    kk = s.eng.calibration_block_marginals()
    assert _blk_err(kk, Si[np_:, np_:]) <= tol
    assert _blk_err(kk, s.eng.get_calibration_marginals()) <= tol
    ids = list(range(0, sc.num_landmarks, 13))
    got = s.eng.landmark_marginals(ids)
    want = _landmark_reference(s, S, ids)
    for q in range(len(ids)):
        assert _blk_err(got[q], want[q]) <= tol, ids[q]
    s.eng.close()


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_landmark_blocks(lm_dim):
    """Landmark blocks against inv(H); one landmark with more than 64 observations (a range of its own);
    ids=None equals the per-id calls bit for bit."""
    sc = scene.make_scene(180, 600, 6, lm_dim=lm_dim, seed=13)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[::9] = 0  # more fixed poses: cond(S) low enough for the check at this size
    # landmark 3 seen from every pose that has it in front of the camera
    x = sc.landmarks[3, :3]
    uv, z = scene.project(sc.gt_poses, np.tile(x, (sc.num_poses, 1)))
    vis = np.nonzero(z > 0.5)[0]
    have = set(sc.obs_pose[sc.obs_lm == 3].tolist()) | {int(sc.lm_ref_pose[3])}
    extra = np.array([p for p in vis if p not in have], dtype=np.uint32)
    assert len(extra) + len(have) > 66, len(extra)
    xo = (uv[extra], extra, np.full(len(extra), 3, dtype=np.uint32))
    s = _engine(sc, lm_dim, pa, pose_pose=True, extra_obs=xo)  # priors keep cond(S) low enough for the check
    assert (s.obs_lm == 3).sum() > 64
    _solve(s)
    S = s.eng.get_S()
    tol = _tol(S)
    ids = [3] + list(range(0, sc.num_landmarks, 17))
    got = s.eng.landmark_marginals(ids)
    want = _landmark_reference(s, S, ids)
    for q in range(len(ids)):
        assert _blk_err(got[q], want[q]) <= tol, ids[q]
    every = s.eng.landmark_marginals(None)
    allids = np.arange(sc.num_landmarks)
    per = s.eng.landmark_marginals(allids)
    assert every.shape == per.shape
    assert np.array_equal(every, per)
    assert s.eng.marginal_stats()["landmark_ms"] > 0
    s.eng.close()


def test_orderings_agree():
    """Revisit route, NATURAL against AUTO: pose and landmark marginals agree, AUTO needs fewer tile products."""
    P = 1200
    sc = scene.make_revisit_scene(P, 5 * P, laps=3, window=12, revisit_frac=0.5, seed=0)
    pa = np.ones(P, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    res = []
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO):
        s = _engine(sc, 1, pa, mode=mode, keep=False)
        _solve(s)
        ids = np.nonzero(pa)[0][::5]
        pm = s.eng.pose_marginals(ids)
        lmm = s.eng.landmark_marginals(None)
        res.append((pm, lmm, s.eng.marginal_stats()))
        s.eng.close()
    (pn, ln, sn), (pu, lu, su) = res
    assert _blk_err(pu, pn) < 1e-10
    assert _blk_err(lu, ln) < 1e-10
    assert su["tile_products"] < sn["tile_products"]
    assert su["levels"] < sn["levels"]


def test_non_interference():
    """Two solves with and without marginals in between: steps, state and calibration marginals bitwise equal."""
    sc = scene.make_scene(70, 300, 6, lm_dim=1, seed=14)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    outs = []
    for ask in (False, True):
        s = _engine(sc, 1, pa, tvs=True)
        rec = []
        for it in range(2):
            s.eng.linearize()
            assert s.eng.solve_gn() == 0
            if ask:
                s.eng.compute_marginals()
                s.eng.pose_marginals([1, 2])
                s.eng.landmark_marginals(None)
            rec.append(s.eng.get_calibration_marginals())
            rec += list(s.eng.get_delta_gn())
            s.eng.compose_step(0.0, 1.0)
            rec += list(s.eng.get_step())
            s.eng.apply_step()
        s.eng.end_solve()
        rec.append(s.eng.get_poses(sc.num_poses)[0])
        rec.append(s.eng.get_landmarks(sc.num_landmarks))
        outs.append(rec)
        s.eng.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_errors():
    sc = scene.make_scene(40, 200, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa)
    eng = s.eng
    with pytest.raises(hipapi.HipError, match="solve_gn"):
        eng.pose_marginals([1])
    _solve(s)
    with pytest.raises(hipapi.HipError, match="not an active pose"):
        eng.pose_marginals([int(sc.anchor_poses[0])])
    with pytest.raises(hipapi.HipError, match="not an active landmark"):
        eng.landmark_marginals([sc.num_landmarks + 5])
    eng.close()
    # a landmark that exists but is inactive (no columns in H)
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    la[7] = 0
    s = _engine(sc, 1, pa, lm_active=la)
    eng = s.eng
    _solve(s)
    with pytest.raises(hipapi.HipError, match="landmark 7 is not an active landmark"):
        eng.landmark_marginals([3, 7])
    assert eng.landmark_marginals([3, 8]).shape == (2, 1, 1)
    assert eng.landmark_marginals(None).shape == (sc.num_landmarks - 1, 1, 1)
    eng.pose_marginals([1])
    eng.close()
    # a pair outside the pattern: a long route, poses far apart share nothing
    sc = scene.make_scene(400, 1200, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, keep=False)
    eng = s.eng
    _solve(s)
    pat = eng.factor_tile_pattern()
    rows = _natural_rows(pa)
    far = [(a, b) for a in range(1, 60) for b in range(sc.num_poses - 1, 150, -1)
           if pa[a] and pa[b] and rows[a] // 64 == (rows[a] + 5) // 64 and rows[b] // 64 == (rows[b] + 5) // 64
           and not pat[rows[b] // 64, rows[a] // 64]]
    assert far, "no pose pair outside the factor's pattern"
    with pytest.raises(hipapi.HipError, match="outside the factor"):
        eng.pose_pair_marginals([far[0][0]], [far[0][1]])
    eng.release_marginals()
    eng.pose_marginals([1])      # recomputed on demand
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="re-linearised"):
        eng.pose_marginals([1])
    with pytest.raises(hipapi.HipError, match="re-linearised"):
        eng.landmark_marginals(None)
    eng.close()


def test_distributed_solve_refused():
    """Collectives hook on two ranks: the distributed solve refuses marginals with a message.  The hooks are
    installed only (set_allreduce with two ranks + set_collectives make the next solve distributed); no
    collective runs."""
    sc = scene.make_scene(40, 200, 6, lm_dim=1, seed=16)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, keep=False)
    s.eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 2)
    s.eng.set_collectives(lambda op, ptr, count, root: 0)
    assert s.eng.solve_is_distributed()
    for call in (s.eng.compute_marginals, lambda: s.eng.pose_marginals([1]), lambda: s.eng.landmark_marginals([0])):
        with pytest.raises(hipapi.HipError, match="distributed solve"):
            call()
    s.eng.close()


def test_sharded_replicated_refuses_landmarks_only():
    """A no-op all-reduce hook on rank 0 of 2 (replicated solve, all landmarks on this rank): pose blocks are
    served and equal the single engine's, landmark blocks are refused."""
    sc = scene.make_scene(40, 200, 6, lm_dim=1, seed=17)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    ref = _engine(sc, 1, pa, keep=False)
    _solve(ref)
    want = ref.eng.pose_marginals([1, 2])
    ref.eng.close()
    s = _engine(sc, 1, pa, keep=False)
    s.eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 2)
    assert not s.eng.solve_is_distributed()
    _solve(s)
    got = s.eng.pose_marginals([1, 2])
    assert _blk_err(got, want) < 1e-12
    with pytest.raises(hipapi.HipError, match="sharded"):
        s.eng.landmark_marginals([0])
    s.eng.close()


def test_calibration_size_4():
    """CalibSize 4 (fx, fy, u0, v0 of camera 0): four calibration rows straddling a tile boundary (21 active poses:
    rows 126..129).  The K x K block equals calibration_marginals() and inv(S); landmark blocks equal inv(H) with
    the intrinsics rows (entry width 4 in the landmark kernel)."""
    sc = scene.make_scene(25, 300, 6, lm_dim=1, seed=18)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[::10] = 0  # the intrinsics need more than the two anchors to be observable
    assert int(pa.sum()) == 21
    s = _engine(sc, 1, pa, calib=4, pose_pose=True)
    _solve(s)
    S = s.eng.get_S()
    n = S.shape[0]
    np_ = n - 4
    assert np_ == 126 and np_ // 64 != (n - 1) // 64
    tol = _tol(S)
    Si = np.linalg.inv(S)
    kk = s.eng.calibration_block_marginals()
    assert kk.shape == (4, 4)
    assert _blk_err(kk, Si[np_:, np_:]) <= tol
    assert _blk_err(kk, s.eng.get_calibration_marginals()) <= tol
    _pose_checks(s, S, tol)
    ids = list(range(0, sc.num_landmarks, 11))
    got = s.eng.landmark_marginals(ids)
    want = _landmark_reference(s, S, ids)
    for q in range(len(ids)):
        assert _blk_err(got[q], want[q]) <= tol, ids[q]
    s.eng.close()


def _sym(S):
    """get_S keeps only the upper block triangle with use_triangular_matrices: mirror it"""
    return np.where(S == 0.0, S.T, S)


def test_pose_size_15_imu_dogleg_through_the_adjuster():
    """PoseSize 15 with IMU residuals, unary priors and binary odometry, solved with dogleg through
    ba::BundleAdjuster (adjuster.py -> ba_capi -> GetPoseCovariance / GetPoseCrossCovariance /
    GetLandmarkCovariance).  15 x 15 pose blocks and pair blocks against inv(S); landmark blocks (6-wide W rows
    inside 15-wide pose blocks) against inv(H)."""
    from ba_amd import adjuster
    P, D = 60, 15
    sc = scene.make_scene(P, 1500, 8, lm_dim=1, seed=2)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    o = adjuster.default_options()
    o.use_dogleg = 1
    o.write_reduced_camera_matrix = 1
    # IMU measurement noise 10x the default: the default's 3e10 pre-integration information on rotation against
    # ~3e3 on the accelerometer bias puts cond(S) above the tolerance rule's 1e-8 (2e5 with the wider noise)
    o.gyro_sigma *= 10.0
    o.accel_sigma *= 10.0
    h = adjuster.BundleAdjuster(1, D)
    h.Init(o)
    pa = np.ones(P, dtype=np.uint8)
    pa[::4] = 0  # fixed poses (root included) and priors on every third pose keep cond(S) low enough for the check
    scene.populate(h, sc, active=pa, imu=True, priors=True, unary_every=3)
    h.Solve(1)
    assert adjuster.RESULT_NAMES[h.summary().result] not in ("FactorizationError", "SolverError")
    ev = h.engine()
    S = _sym(ev.get_S())
    rows = _natural_rows(pa, D)
    assert S.shape == (int(pa.sum()) * D,) * 2
    tol = _tol(S)
    Si = np.linalg.inv(S)
    for i in np.nonzero(pa)[0]:
        got = h.pose_covariance(i)
        assert got.shape == (D, D)
        r = rows[i]
        assert _blk_err(got, Si[r:r + D, r:r + D]) <= tol, i
    for a in range(1, P - 1):  # consecutive active poses: an IMU residual couples them
        if pa[a] and pa[a + 1]:
            got = h.pose_covariance(a, a + 1)
            ra, rb = rows[a], rows[a + 1]
            assert _blk_err(got, Si[ra:ra + D, rb:rb + D]) <= tol, a
    with pytest.raises(RuntimeError, match="unavailable"):
        h.pose_covariance(0)  # fixed
    # landmark blocks: the engine's residuals are the populated observations in order
    s = Setup()
    s.eng, s.sc, s.pa, s.lm_dim, s.tvs, s.D, s.K = ev, sc, pa, 1, False, D, 0
    # (AddProjectionResidual rejects the reference frame's own observation: it only sets z_ref)
    acc = sc.obs_pose != sc.lm_ref_pose[sc.obs_lm]
    s.obs_pose, s.obs_lm = np.asarray(sc.obs_pose[acc], dtype=np.int64), np.asarray(sc.obs_lm[acc], dtype=np.int64)
    ids = list(range(0, sc.num_landmarks, 97))
    want = _landmark_reference(s, S, ids)
    for q, l in enumerate(ids):
        got = h.landmark_covariance(l)
        assert got.shape == (1, 1)
        assert _blk_err(got, want[q]) <= tol, l
    assert np.array_equal(ev.landmark_marginals(ids)[:, 0, 0], [h.landmark_covariance(l)[0, 0] for l in ids])
    with pytest.raises(RuntimeError, match="unavailable"):
        h.landmark_covariance(sc.num_landmarks + 3)


def test_scale_configs1():
    """configs[1] (1 000 poses, n = 5 988): finite positive sigmas, symmetric positive definite pose blocks, and 20
    pose blocks against multi-RHS solves with the kept S."""
    sc = scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa)
    _solve(s)
    eng = s.eng
    act = np.nonzero(pa)[0]
    cov = eng.pose_marginals(act)
    assert np.all(np.isfinite(cov))
    assert np.abs(cov - np.transpose(cov, (0, 2, 1))).max() <= 1e-12 * np.abs(cov).max()
    assert np.all(np.linalg.eigvalsh(0.5 * (cov + np.transpose(cov, (0, 2, 1)))) > 0)
    lm = eng.landmark_marginals(None)
    assert lm.shape == (sc.num_landmarks, 1, 1) and np.all(np.isfinite(lm)) and np.all(lm > 0)
    S = eng.get_S()
    rows = _natural_rows(pa)
    pick = act[np.random.default_rng(1).choice(len(act), 20, replace=False)]
    E = np.zeros((S.shape[0], 20 * 6))
    for q, p in enumerate(pick):
        E[rows[p]:rows[p] + 6, 6 * q:6 * q + 6] = np.eye(6)
    X = np.linalg.solve(S, E)
    got = eng.pose_marginals(pick)
    for q, p in enumerate(pick):
        want = X[rows[p]:rows[p] + 6, 6 * q:6 * q + 6]
        assert _blk_err(got[q], want) <= 1e-8, p
    st = eng.marginal_stats()
    assert st["levels"] > 1 and st["tile_products"] > st["factor_tile_products"]
    eng.close()
