"""Joint covariances of mixed pose, calibration and landmark sets on the MI355X (ba_hip_get_joint_state_marginals,
k_jointcov.hip: k_joint_seed, k_joint_rhs, k_joint_lmdiag): the block of the inverse of the full system
[[U, W], [W^T, V]] over the requested parameters, cross blocks included, against inv(H) with
H = [[S + W V^-1 W^T, W], [W^T, V]] over the requested landmarks, built from the kept S and the engine's Jacobians
(the construction of test_marginals_gpu._landmark_reference, the whole inverse kept).  Every comparison is in
correlation units, err = max |got - want|_ab / (d_a d_b) with d = sqrt(diag(want)), under
tol = max(1e-9, 4.5 eps cond(S))."""
import gc

import numpy as np
import pytest

from ba_amd import hipapi, scene
import joint_state_cases as jc
import leverage_cases as lc

pytestmark = pytest.mark.gpu


def _fixed(sc, more=()):
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[list(more)] = 0
    return pa


def _accepted(sc, lm_dim):
    """(z, pose, lm) of the residuals the engine accepts: LmSize 1 drops the reference frame's own observation"""
    sel = np.ones(len(sc.obs_pose), dtype=bool)
    if lm_dim == 1:
        sel[::sc.obs_per_landmark + 1] = False
    return sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel]


class Ref:
    """inv(H) blocks of one solved engine: J once, a request's block on demand"""

    def __init__(self, s):
        self.s = s
        self.S = s.eng.get_S()
        self.tol = lc.tolerance(self.S)
        self.J, self.n = lc.engine_jacobian(s)
        assert self.n == self.S.shape[0]

    def block(self, poses, lms, calib=False):
        s = self.s
        lm_cols = jc.request_columns(s.lm_dim, s.D, s.K, s.pa, s.la, [], lms)
        Jl = self.J[:, lm_cols]
        W = self.J[:, :self.n].T @ Jl
        V = Jl.T @ Jl
        U = self.S + W @ np.linalg.solve(V, W.T) if len(lm_cols) else self.S
        Hi = np.linalg.inv(np.block([[U, W], [W.T, V]]))
        sel = list(jc.request_columns(s.lm_dim, s.D, s.K, s.pa, s.la, poses, [], include_calibration=calib))
        sel += list(self.n + np.arange(len(lm_cols)))
        return Hi[np.ix_(sel, sel)]


def _check(ref, poses, lms, calib=False, what=""):
    """err <= tol, bitwise symmetric, the same bits on a second call"""
    eng = ref.s.eng
    got = eng.joint_state_marginals(poses, lms, include_calibration=calib)
    want = ref.block(poses, lms, calib)
    assert got.shape == want.shape
    err = jc.corr_err(got, want)
    print("%s: %d poses, %d landmarks, M = %d: err %.3g tol %.3g" % (what, len(poses), len(lms), len(got), err, ref.tol))
    assert err <= ref.tol
    assert np.array_equal(got, got.T)
    assert np.array_equal(got, eng.joint_state_marginals(poses, lms, include_calibration=calib))
    return got, want


def _blocks_close(a, b, tol):
    d = np.sqrt(np.diag(b))
    return (np.abs(a - b) / np.outer(d, d)).max() <= tol


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_fixed_poses_and_pose_pose_terms(lm_dim):
    sc = scene.make_scene(83, 500, 6, lm_dim=lm_dim, seed=11)
    pa = _fixed(sc, [9, 40])
    s = lc.engine(sc, lm_dim, pa, pose_pose=True)
    lc.solve(s)
    eng = s.eng
    ref = Ref(s)
    assert ref.S.shape[0] % 64 != 0
    LM, rows = lm_dim, lc.natural_rows(pa)
    act = [int(p) for p in np.nonzero(pa)[0]]
    straddle = [p for p in act if rows[p] // 64 != (rows[p] + 5) // 64]
    spread = []   # landmarks seen from poses in at least three tile rows
    for l in range(sc.num_landmarks):
        ps = set(s.obs_pose[s.obs_lm == l].tolist()) | ({int(sc.lm_ref_pose[l])} if LM == 1 else set())
        if len({rows[p] // 64 for p in ps if pa[p]}) >= 3:
            spread.append(l)
    assert straddle and spread
    before = eng.marginal_stats()
    assert before["store_bytes"] == 0
    results = {}
    many_p, many_l = act[::-1][::9], list(range(0, sc.num_landmarks, 23))[::-1]
    assert len(many_p) * 6 + len(many_l) * LM > 64
    for name, poses, lms in (("one and one", [act[0]], [0]),
                             ("straddling pose, spread landmark", [straddle[0]], [spread[0]]),
                             ("caller's order, two column blocks", many_p, many_l),
                             ("landmarks only", [], [spread[1]] + [l for l in (7, 2, 11) if l != spread[1]][:2])):
        results[name] = (poses, lms) + _check(ref, poses, lms, what="LM %d, %s" % (LM, name))
        st = eng.joint_state_stats()
        assert st["landmark_columns"] == LM * len(lms) and st["incidences"] >= len(lms) and st["seed_tiles"] >= 1
        assert st["rhs_ms"] > 0
        assert eng.joint_marginal_stats()["columns"] == len(poses) * 6 + LM * len(lms)
    # poses only: one code path with joint_marginals
    ids = [act[-1], straddle[0], act[3]]
    assert np.array_equal(eng.joint_state_marginals(ids, []), eng.joint_marginals(ids))
    assert eng.joint_state_stats()["landmark_columns"] == 0
    assert eng.marginal_stats() == before
    # the cross blocks are not small
    poses, lms, got, want = results["caller's order, two column blocks"]
    c0 = 6 * len(poses)
    corr = want / np.sqrt(np.outer(np.diag(want), np.diag(want)))
    print("LM %d: largest pose-landmark correlation %.2f, landmark-landmark %.2f"
          % (LM, np.abs(corr[:c0, c0:]).max(), np.abs(corr[c0:, c0:] - np.eye(len(want) - c0)).max()))
    assert np.abs(corr[:c0, c0:]).max() > 0.05
    # against the getters that serve the diagonal blocks
    lmm = eng.landmark_marginals(lms)
    for q in range(len(lms)):
        sl = slice(c0 + LM * q, c0 + LM * (q + 1))
        assert _blocks_close(got[sl, sl], lmm[q], 2 * ref.tol), lms[q]
    assert _blocks_close(got[:c0, :c0], eng.joint_marginals(poses), 2 * ref.tol)
    eng.close()


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_landmark_with_more_than_64_observations(lm_dim):
    sc = scene.make_scene(180, 600, 6, lm_dim=lm_dim, seed=13)
    pa = _fixed(sc)
    pa[::9] = 0
    x = sc.landmarks[3, :3]
    uv, z = scene.project(sc.gt_poses, np.tile(x, (sc.num_poses, 1)))
    vis = np.nonzero(z > 0.5)[0]
    have = set(sc.obs_pose[sc.obs_lm == 3].tolist()) | {int(sc.lm_ref_pose[3])}
    extra = np.array([p for p in vis if p not in have], dtype=np.uint32)
    zz, pp, ll = _accepted(sc, lm_dim)
    obs = (np.concatenate([zz, uv[extra]]), np.concatenate([pp, extra]),
           np.concatenate([ll, np.full(len(extra), 3, dtype=ll.dtype)]))
    s = lc.engine(sc, lm_dim, pa, pose_pose=True, obs=obs)
    assert (s.obs_lm == 3).sum() > 64
    lc.solve(s)
    ref = Ref(s)
    act = [int(p) for p in np.nonzero(pa)[0]]
    rp = int(sc.lm_ref_pose[3])
    near = rp if pa[rp] else min(act, key=lambda p: abs(p - rp))
    far = act[-1] if abs(act[-1] - near) > abs(act[0] - near) else act[0]
    _check(ref, [near, far], [3, 100, 250, 599], what="LM %d, long track" % lm_dim)
    assert s.eng.joint_state_stats()["incidences"] > 64
    s.eng.close()


def test_calibration_rows_with_tvs():
    sc = scene.make_scene(44, 300, 6, lm_dim=1, seed=12)
    pa = _fixed(sc)
    s = lc.engine(sc, 1, pa, tvs=True, pose_pose=True)
    lc.solve(s)
    ref = Ref(s)
    n = ref.S.shape[0]
    assert (n - 6) // 64 != (n - 1) // 64, "calibration rows do not straddle a tile"
    act = [int(p) for p in np.nonzero(pa)[0]]
    lms = list(range(0, sc.num_landmarks, 31))
    got, _ = _check(ref, [act[2], act[-1]], lms, calib=True, what="DoTvs")
    assert got.shape == (12 + 6 + len(lms),) * 2
    _check(ref, [], lms[:3], calib=True, what="DoTvs, no pose")
    _check(ref, [act[5]], lms[:3], calib=False, what="DoTvs, calibration not asked for")
    s.eng.close()


def test_masks_and_orderings():
    """Three masked translation parameters of the first active pose; NATURAL, AUTO and a reversed pose order."""
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    pa = _fixed(sc)
    first = int(np.nonzero(pa)[0][0])
    masks = np.zeros(sc.num_poses, dtype=np.uint16)
    masks[first] = 0x7
    rev = np.arange(int(pa.sum()), dtype=np.uint32)[::-1]
    poses, lms = [first, int(np.nonzero(pa)[0][-1])], list(range(0, sc.num_landmarks, 7))
    res = []
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO, hipapi.ORDER_USER):
        s = lc.engine(sc, 1, pa, mode=mode, pose_pose=True, masks=masks, perm=rev if mode == hipapi.ORDER_USER else None)
        lc.solve(s)
        ref = Ref(s)
        got, want = _check(ref, poses, lms, what="masks, ordering mode %d" % mode)
        res.append((got, want, ref.tol))
        s.eng.close()
    for got, want, tol in res[1:]:
        d = np.sqrt(np.diag(want))
        diff = (np.abs(got - res[0][0]) / np.outer(d, d)).max()
        print("orderings: difference to natural order %.3g (tol %.3g)" % (diff, tol))
        assert diff <= 2 * tol


def test_landmark_without_observations_and_a_duplicate():
    sc = scene.make_scene(40, 200, 6, lm_dim=3, seed=15)
    pa = _fixed(sc)
    zz, pp, ll = _accepted(sc, 3)
    keep = ll != 5                                   # landmark 5: active, no residual at all
    dup = int(np.nonzero(ll == 8)[0][2])             # landmark 8: one observation twice (same pose, same landmark)
    idx = np.concatenate([np.nonzero(keep)[0], [dup]])
    s = lc.engine(sc, 3, pa, pose_pose=True, obs=(zz[idx], pp[idx], ll[idx]))
    lc.solve(s)
    eng = s.eng
    act = [int(p) for p in np.nonzero(pa)[0]]
    got = eng.joint_state_marginals([act[0], act[-1]], [4, 5, 8])
    blk = got[15:18, 15:18]                          # columns: 12 of the poses, then landmarks 4, 5, 8
    assert np.array_equal(blk, 1e6 * np.eye(3))
    assert not got[15:18, :15].any() and not got[15:18, 18:].any() and not got[:15, 15:18].any()
    assert np.array_equal(got, got.T)
    # the reference without the unobserved landmark (its V is zero: H over it is singular)
    ref = Ref(s)
    _check(ref, [act[0], act[-1]], [4, 8], what="duplicated observation")
    keep2 = [c for c in range(len(got)) if not 15 <= c < 18]
    assert np.array_equal(got[np.ix_(keep2, keep2)], eng.joint_state_marginals([act[0], act[-1]], [4, 8]))
    # the unobserved landmark alone: an empty reach, no substitution at all
    alone = eng.joint_state_marginals([], [5])
    assert np.array_equal(alone, 1e6 * np.eye(3))
    st = eng.joint_marginal_stats()
    assert st["reach_tiles"] == 0 and st["levels"] == 0 and eng.joint_state_stats()["incidences"] == 0
    eng.close()


def test_errors_and_refusals():
    e0 = hipapi.Engine(0, 6)
    with pytest.raises(hipapi.HipError, match="LmSize 0"):
        e0.joint_state_marginals([1], [0])
    e0.close()
    sc = scene.make_scene(40, 200, 6, lm_dim=3, seed=15)
    pa = _fixed(sc)
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    la[7] = 0
    s = lc.engine(sc, 3, pa, lm_active=la)
    eng = s.eng
    with pytest.raises(hipapi.HipError, match="solve_gn"):
        eng.joint_state_marginals([1], [0])
    lc.solve(s)
    good = eng.joint_state_marginals([1, 2], [0, 3])

    def still_works():
        assert np.array_equal(eng.joint_state_marginals([1, 2], [0, 3]), good)

    for poses, lms, msg in (([1, int(sc.anchor_poses[0])], [0], "is not an active pose"),
                            ([sc.num_poses + 3], [0], "is not an active pose"),
                            ([1], [7], "landmark 7 is not an active landmark"),
                            ([1], [sc.num_landmarks], "is not an active landmark"),
                            ([1, 2, 1], [0], "pose 1 is repeated"),
                            ([1], [3, 0, 3], "landmark 3 is repeated"),
                            ([], [], "no pose")):
        with pytest.raises(hipapi.HipError, match=msg):
            eng.joint_state_marginals(poses, lms)
        still_works()
    with pytest.raises(hipapi.HipError, match="include_calibration"):
        eng.joint_state_marginals([1], [0], include_calibration=True)
    act = [int(p) for p in np.nonzero(pa)[0]]
    lms = [l for l in range(sc.num_landmarks) if la[l]]
    assert len(act) == 38
    with pytest.raises(hipapi.HipError, match="513 columns requested, the limit is BA_HIP_JOINT_MAX_COLUMNS \\(512\\)"):
        eng.joint_state_marginals(act, lms[:95])
    full = eng.joint_state_marginals(act, lms[:94])   # 510 columns: eight column blocks
    assert full.shape == (510, 510) and np.array_equal(full, full.T) and np.all(np.isfinite(full))
    assert np.array_equal(full[:228, :228], eng.joint_marginals(act))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_joint_state_marginals(eng.h, 1, None, 0, 0, None, None))
    ids = np.array([0], dtype=np.uint32)
    out = np.zeros((3, 3))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_joint_state_marginals(eng.h, 0, None, 0, 1, None, hipapi._p(out, hipapi.dp)))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_joint_state_marginals(eng.h, 0, None, 0, 1, hipapi._p(ids, hipapi.u32p), None))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_joint_state_stats(eng.h, None))
    still_works()
    # after ba_hip_linearize, after a PCG solve
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="re-linearised"):
        eng.joint_state_marginals([1], [0])
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8)
    assert eng.solve_gn() == 0
    with pytest.raises(hipapi.HipError, match="PCG"):
        eng.joint_state_marginals([1], [0])
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    lc.solve(s)
    still_works()
    eng.close()
    # sharded replicated engine: landmarks refused, poses served; the distributed solve refuses everything
    s = lc.engine(sc, 3, pa)
    s.eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 2)
    assert not s.eng.solve_is_distributed()
    lc.solve(s)
    with pytest.raises(hipapi.HipError, match="sharded"):
        s.eng.joint_state_marginals([1], [0])
    assert np.array_equal(s.eng.joint_state_marginals([1, 30], []), s.eng.joint_marginals([1, 30]))
    s.eng.close()
    # (the hooks of the distributed solve installed, no collective runs: the engine of test_marginals_gpu, which
    # does not keep the reduced system)
    from test_marginals_gpu import _engine
    sc = scene.make_scene(40, 200, 6, lm_dim=1, seed=17)
    s = _engine(sc, 1, _fixed(sc), keep=False)
    s.eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 2)
    s.eng.set_collectives(lambda op, ptr, count, root: 0)
    assert s.eng.solve_is_distributed()
    with pytest.raises(hipapi.HipError, match="distributed solve"):
        s.eng.joint_state_marginals([1], [0])
    s.eng.close()


def test_non_interference():
    """Steps, the next solve, pose_marginals and joint_marginals of a run that calls the new getter are bitwise those
    of a run that never does."""
    sc = scene.make_scene(70, 300, 6, lm_dim=1, seed=14)
    pa = _fixed(sc)
    act = [int(p) for p in np.nonzero(pa)[0]]
    ids, lms = [act[-1], act[0], act[20]], [0, 150, 299, 17]
    outs = []
    for ask in (False, True):
        s = lc.engine(sc, 1, pa, tvs=True)
        rec = []
        for it in range(2):
            lc.solve(s)
            if ask:
                before = s.eng.marginal_stats()
                j1 = s.eng.joint_state_marginals(ids, lms, include_calibration=True)
                s.eng.joint_state_marginals([act[3]], [5])
                assert np.array_equal(j1, s.eng.joint_state_marginals(ids, lms, include_calibration=True))
                assert s.eng.marginal_stats() == before
                if it == 0:
                    assert before["selinv_ms"] == 0 and before["store_bytes"] == 0
            rec.append(s.eng.joint_marginals(ids, include_calibration=True))
            rec.append(s.eng.pose_marginals(ids))
            rec.append(s.eng.landmark_marginals(lms))
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


def test_pose_size_15_through_the_adjuster():
    """The scene of test_marginals_gpu.test_pose_size_15_imu_dogleg_through_the_adjuster: GetJointCovariance against
    the getters that serve its diagonal blocks; no dense reference."""
    from ba_amd import adjuster
    from test_marginals_gpu import _sym, _tol
    P, D = 60, 15
    sc = scene.make_scene(P, 1500, 8, lm_dim=1, seed=2)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    o = adjuster.default_options()
    o.use_dogleg = 1
    o.write_reduced_camera_matrix = 1
    o.gyro_sigma *= 10.0
    o.accel_sigma *= 10.0
    h = adjuster.BundleAdjuster(1, D)
    h.Init(o)
    pa = np.ones(P, dtype=np.uint8)
    pa[::4] = 0
    scene.populate(h, sc, active=pa, imu=True, priors=True, unary_every=3)
    h.Solve(1)
    assert adjuster.RESULT_NAMES[h.summary().result] not in ("FactorizationError", "SolverError")
    ev = h.engine()
    tol = _tol(_sym(ev.get_S()))
    poses, lms = [57, 1, 30], list(range(0, sc.num_landmarks, 211))
    got = h.GetJointCovariance(poses, lms)
    c0 = D * len(poses)
    assert got.shape == (c0 + len(lms),) * 2 and np.array_equal(got, got.T)
    assert np.array_equal(got, ev.joint_state_marginals(poses, lms))
    assert _blocks_close(got[:c0, :c0], h.GetJointPoseCovariance(poses), 2 * tol)
    for q, l in enumerate(lms):
        assert _blocks_close(got[c0 + q:c0 + q + 1, c0 + q:c0 + q + 1], h.landmark_covariance(l), 2 * tol), l
    assert np.abs(got[:c0, c0:]).max() > 0
    cross = h.GetPoseLandmarkCrossCovariance(30, lms[2])
    # (the same block out of a request with another reach: the Gram product groups other rows, so not the same bits)
    dd = np.sqrt(np.diag(got))
    assert cross.shape == (D, 1)
    assert (np.abs(cross[:, 0] - got[2 * D:3 * D, c0 + 2]) / (dd[2 * D:3 * D] * dd[c0 + 2])).max() <= 2 * tol
    with pytest.raises(RuntimeError, match="unavailable"):
        h.GetJointCovariance([1, 0], lms)  # pose 0 is fixed
    with pytest.raises(RuntimeError, match="unavailable"):
        h.GetPoseLandmarkCrossCovariance(1, sc.num_landmarks + 3)
    del h
    gc.collect()


def test_ownership():
    live = hipapi.device_bytes_live
    base = live()
    sc = scene.make_scene(12, 60, 4, lm_dim=3, seed=11)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[:2] = 0
    s = lc.engine(sc, 3, pa, pose_pose=True)
    lc.solve(s)
    solved = live()
    s.eng.joint_state_marginals([2, 7], [0, 30, 59])
    assert live() > solved
    s.eng.release_marginals()
    assert live() == solved
    s.eng.joint_state_marginals([2, 7], [0, 30, 59])
    s.eng.close()
    assert live() == base
