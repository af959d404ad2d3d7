"""Joint covariances of arbitrary pose sets on the MI355X (ba_hip_get_joint_marginals, k_jointcov.hip): the
M x M block of S^-1 over any active poses, from a forward substitution over the reach and a Gram product,
against dense inverses of the kept S, against the selected-inverse getters where those serve the block, and
for what it must leave alone.  Tolerance: max(1e-9, 4.5 eps cond(S)) relative to the largest entry of the
reference joint block; the Gram form's own error on these systems stays below 1.3e-13."""
import numpy as np
import pytest

from ba_amd import hipapi, scene
from test_marginals_gpu import EPS, _blk_err, _engine, _natural_rows, _solve, _sym, _tol

pytestmark = pytest.mark.gpu


def _rows_of(rows, ids, D=6, border=()):
    return np.array([rows[p] + x for p in ids for x in range(D)] + list(border), dtype=np.int64)


def _ref_block(Si, rows, ids, D=6, border=()):
    r = _rows_of(rows, ids, D, border)
    return Si[np.ix_(r, r)]


def _far_pairs(eng, sc, pa):
    """pairs whose block lies outside the factor's tile pattern, found as test_marginals_gpu.test_errors does"""
    pat = eng.factor_tile_pattern()
    rows = _natural_rows(pa)
    return [(a, b) for a in range(1, 60) for b in range(sc.num_poses - 1, 150, -1)
            if pa[a] and pa[b] and rows[a] // 64 == (rows[a] + 5) // 64 and rows[b] // 64 == (rows[b] + 5) // 64
            and not pat[rows[b] // 64, rows[a] // 64]]


def _plan_counts(pat, tiles):
    """reach tiles and tile products per 64 columns of the host plan (jointcov.h) on the lower pattern `pat`"""
    nt = pat.shape[0]
    inr = np.zeros(nt, dtype=bool)
    for t in tiles:
        j = int(t)
        while j < nt and not inr[j]:
            inr[j] = True
            below = np.nonzero(pat[j + 1:, j])[0]
            j = j + 1 + int(below[0]) if len(below) else nt
    idx = np.nonzero(inr)[0]
    sub = np.tril(pat[np.ix_(idx, idx)] != 0, -1)
    return len(idx), int(sub.sum()) + len(idx)


def _against_getters(eng, ids, joint, tol, D=6):
    """diagonal blocks equal pose_marginals; the pairs the selected inverse serves equal pose_pair_marginals"""
    pm = eng.pose_marginals(ids)
    scale = np.abs(joint).max()
    for i in range(len(ids)):
        got = joint[i * D:(i + 1) * D, i * D:(i + 1) * D]
        assert np.abs(got - pm[i]).max() <= 2 * tol * scale, ids[i]
    served = 0
    for i in range(len(ids)):
        for j in range(len(ids)):
            if i == j:
                continue
            try:
                pr = eng.pose_pair_marginals([ids[i]], [ids[j]])[0]
            except hipapi.HipError as ex:
                assert "outside the factor" in str(ex)
                continue
            served += 1
            got = joint[i * D:(i + 1) * D, j * D:(j + 1) * D]
            assert np.abs(got - pr).max() <= 2 * tol * scale, (ids[i], ids[j])
    return served


def test_far_pair_outside_the_pattern():
    """The pair the selected inverse refuses: its joint block equals inv(S), and the cross block is not small."""
    sc = scene.make_scene(400, 1200, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, keep=True)
    eng = s.eng
    _solve(s)
    far = _far_pairs(eng, sc, pa)
    assert far, "no pose pair outside the factor's pattern"
    a, b = far[0]
    before = eng.marginal_stats()
    joint = eng.joint_marginals([a, b])
    assert eng.marginal_stats() == before and before["selinv_ms"] == 0 and before["store_bytes"] == 0
    with pytest.raises(hipapi.HipError, match="outside the factor"):
        eng.pose_pair_marginals([a], [b])
    S = eng.get_S()
    tol = _tol(S)
    Si = np.linalg.inv(S)
    rows = _natural_rows(pa)
    want = _ref_block(Si, rows, [a, b])
    err = _blk_err(joint, want)
    cross = np.abs(joint[:6, 6:]).max() / np.abs(joint).max()
    print("far pair (%d, %d): err %.3g tol %.3g cross/max %.3g" % (a, b, err, tol, cross))
    assert err <= tol
    assert cross >= 1e-3
    assert np.array_equal(joint, joint.T)
    # pose 1 and the last pose, the pair of the issue
    last = int(np.nonzero(pa)[0][-1])
    j2 = eng.joint_marginals([1, last])
    assert _blk_err(j2, _ref_block(Si, rows, [1, last])) <= tol
    st = eng.joint_marginal_stats()
    nt = (S.shape[0] + 63) // 64
    assert st["columns"] == 12 and 0 < st["reach_tiles"] <= nt and st["levels"] >= 1
    assert st["solve_ms"] > 0 and st["gram_ms"] > 0 and st["workspace_bytes"] > 0
    assert _against_getters(eng, [a, b], joint, tol) == 0
    eng.close()


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_fixed_poses_and_pose_pose_terms(lm_dim):
    """LmSize 1 and 3, fixed poses, pose-pose terms, n no multiple of 64; sets of one, two, neighbouring (a pose
    straddling a tile boundary) and many poses, in an order of the caller's."""
    sc = scene.make_scene(83, 500, 6, lm_dim=lm_dim, seed=11)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[[9, 40]] = 0
    s = _engine(sc, lm_dim, pa, pose_pose=True)
    _solve(s)
    eng = s.eng
    S = eng.get_S()
    assert S.shape[0] % 64 != 0
    tol = _tol(S)
    Si = np.linalg.inv(S)
    rows = _natural_rows(pa)
    act = [int(p) for p in np.nonzero(pa)[0]]
    straddle = [p for p in act if rows[p] // 64 != (rows[p] + 5) // 64]
    assert straddle
    served = 0
    for ids in ([act[0]], [act[-1], act[0]], [straddle[0], act[5]], [act[3], act[4], act[5]], act[::-1][::7], act[:64]):
        joint = eng.joint_marginals(ids)
        assert joint.shape == (6 * len(ids),) * 2
        err = _blk_err(joint, _ref_block(Si, rows, ids))
        print("lm_dim %d, %d poses: err %.3g tol %.3g" % (lm_dim, len(ids), err, tol))
        assert err <= tol, ids
        assert np.array_equal(joint, joint.T)
        if len(ids) <= 12:
            served += _against_getters(eng, ids, joint, tol)
    assert served > 0
    eng.close()


def test_calibration_rows_with_tvs():
    """DoTvs with include_calibration: the border straddles a tile; the K rows come last."""
    sc = scene.make_scene(44, 300, 6, lm_dim=1, seed=12)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, tvs=True, pose_pose=True)
    _solve(s)
    eng = s.eng
    S = eng.get_S()
    n = S.shape[0]
    np_ = n - 6
    assert np_ // 64 != (n - 1) // 64, "calibration rows do not straddle a tile"
    tol = _tol(S)
    Si = np.linalg.inv(S)
    rows = _natural_rows(pa)
    act = [int(p) for p in np.nonzero(pa)[0]]
    border = list(range(np_, n))
    for ids in ([act[2], act[-1]], [], act[::5]):
        joint = eng.joint_marginals(ids, include_calibration=True)
        assert joint.shape == (6 * len(ids) + 6,) * 2
        assert _blk_err(joint, _ref_block(Si, rows, ids, border=border)) <= tol
        assert np.abs(joint[-6:, -6:] - eng.calibration_block_marginals()).max() <= 2 * tol * np.abs(joint).max()
    without = eng.joint_marginals([act[2], act[-1]])
    assert _blk_err(without, _ref_block(Si, rows, [act[2], act[-1]])) <= tol
    eng.close()


def test_calibration_size_4():
    sc = scene.make_scene(25, 300, 6, lm_dim=1, seed=18)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[::10] = 0
    s = _engine(sc, 1, pa, calib=4, pose_pose=True)
    _solve(s)
    eng = s.eng
    S = eng.get_S()
    n = S.shape[0]
    assert n - 4 == 126
    tol = _tol(S)
    Si = np.linalg.inv(S)
    rows = _natural_rows(pa)
    act = [int(p) for p in np.nonzero(pa)[0]]
    ids = [act[-1], act[0], act[10]]
    joint = eng.joint_marginals(ids, include_calibration=True)
    assert joint.shape == (22, 22)
    assert _blk_err(joint, _ref_block(Si, rows, ids, border=range(126, 130))) <= tol
    _against_getters(eng, ids, joint[:18, :18], tol)
    eng.close()


def test_pose_size_15_imu_through_the_adjuster():
    """PoseSize 15 with IMU residuals through ba::BundleAdjuster: GetJointPoseCovariance equals the engine-level
    call bit for bit and inv(S) within the tolerance."""
    from ba_amd import adjuster
    P, D = 60, 15
    sc = scene.make_scene(P, 1500, 8, lm_dim=1, seed=2)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    o = adjuster.default_options()
    o.use_dogleg = 1
    o.write_reduced_camera_matrix = 1
    o.gyro_sigma *= 10.0   # as test_marginals_gpu: keeps cond(S) inside the tolerance rule
    o.accel_sigma *= 10.0
    h = adjuster.BundleAdjuster(1, D)
    h.Init(o)
    pa = np.ones(P, dtype=np.uint8)
    pa[::4] = 0
    scene.populate(h, sc, active=pa, imu=True, priors=True, unary_every=3)
    h.Solve(1)
    assert adjuster.RESULT_NAMES[h.summary().result] not in ("FactorizationError", "SolverError")
    ev = h.engine()
    S = _sym(ev.get_S())
    rows = _natural_rows(pa, D)
    tol = _tol(S)
    Si = np.linalg.inv(S)
    ids = [57, 1, 30, 31]
    got = h.GetJointPoseCovariance(ids)
    assert got.shape == (60, 60)
    assert np.array_equal(got, ev.joint_marginals(ids))
    assert _blk_err(got, _ref_block(Si, rows, ids, D)) <= tol
    assert np.abs(got[30:45, 45:60] - h.pose_covariance(30, 31)).max() <= 2 * tol * np.abs(got).max()
    with pytest.raises(RuntimeError, match="unavailable"):
        h.GetJointPoseCovariance([1, 0])  # pose 0 is fixed


def test_orderings_agree():
    """Revisit route, NATURAL against AUTO: the joint block is the one of natural order either way."""
    P = 300
    sc = scene.make_revisit_scene(P, 5 * P, laps=3, window=12, revisit_frac=0.5, seed=0)
    pa = np.ones(P, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    act = [int(p) for p in np.nonzero(pa)[0]]
    ids = [act[1], act[-1], act[len(act) // 2], act[len(act) // 3]]
    res = []
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO):
        s = _engine(sc, 1, pa, mode=mode, keep=True)
        _solve(s)
        res.append((s.eng.joint_marginals(ids), s.eng.get_S(), s.eng.joint_marginal_stats()))
        s.eng.close()
    (jn, S, sn), (ju, _, su) = res
    tol = _tol(S)
    Si = np.linalg.inv(S)
    want = _ref_block(Si, _natural_rows(pa), ids)
    print("orderings: natural err %.3g auto err %.3g between %.3g tol %.3g; reach %d / %d levels %d / %d"
          % (_blk_err(jn, want), _blk_err(ju, want), _blk_err(ju, jn), tol, sn["reach_tiles"], su["reach_tiles"],
             sn["levels"], su["levels"]))
    assert _blk_err(jn, want) <= tol and _blk_err(ju, want) <= tol
    assert _blk_err(ju, jn) <= tol


def test_determinism_and_non_interference():
    """Two calls give the same bits; steps, state, calibration marginals and pose marginals are bitwise those of
    a run that never asks; a joint call on a fresh factor leaves marginal_stats alone (no selected inverse)."""
    sc = scene.make_scene(70, 300, 6, lm_dim=1, seed=14)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    act = [int(p) for p in np.nonzero(pa)[0]]
    ids = [act[-1], act[0], act[20]]
    outs = []
    for ask in (False, True):
        s = _engine(sc, 1, pa, tvs=True)
        rec = []
        for it in range(2):
            s.eng.linearize()
            assert s.eng.solve_gn() == 0
            if ask:
                before = s.eng.marginal_stats()
                j1 = s.eng.joint_marginals(ids, include_calibration=True)
                j2 = s.eng.joint_marginals(ids, include_calibration=True)
                assert np.array_equal(j1, j2) and np.array_equal(j1, j1.T)
                s.eng.joint_marginals([act[3]])
                j3 = s.eng.joint_marginals(ids, include_calibration=True)  # after a request of another shape
                assert np.array_equal(j1, j3)
                assert s.eng.marginal_stats() == before
                if it == 0:
                    assert before["selinv_ms"] == 0 and before["store_bytes"] == 0
            rec.append(s.eng.pose_marginals(ids))
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
        eng.joint_marginals([1, 2])
    _solve(s)
    good = eng.joint_marginals([1, 2])

    def still_works():
        assert np.array_equal(eng.joint_marginals([1, 2]), good)

    with pytest.raises(hipapi.HipError, match="is not an active pose"):
        eng.joint_marginals([1, int(sc.anchor_poses[0])])
    still_works()
    with pytest.raises(hipapi.HipError, match="is not an active pose"):
        eng.joint_marginals([sc.num_poses + 3])
    still_works()
    with pytest.raises(hipapi.HipError, match="repeated"):
        eng.joint_marginals([1, 2, 1])
    still_works()
    with pytest.raises(hipapi.HipError, match="include_calibration"):
        eng.joint_marginals([1, 2], include_calibration=True)
    still_works()
    with pytest.raises(hipapi.HipError, match="no pose"):
        eng.joint_marginals([])
    act = [int(p) for p in np.nonzero(pa)[0]]
    assert len(act) * 6 < hipapi.JOINT_MAX_COLUMNS
    eng.close()
    # too many columns: 86 poses of 6 rows = 516 > 512
    sc = scene.make_scene(100, 400, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, keep=False)
    eng = s.eng
    _solve(s)
    act = [int(p) for p in np.nonzero(pa)[0]]
    with pytest.raises(hipapi.HipError, match="BA_HIP_JOINT_MAX_COLUMNS \\(512\\)"):
        eng.joint_marginals(act[:86])
    full = eng.joint_marginals(act[:85])  # 510 columns: eight column blocks
    assert full.shape == (510, 510) and np.array_equal(full, full.T)
    pm = eng.pose_marginals(act[:85])
    for q in range(85):
        assert np.abs(full[6 * q:6 * q + 6, 6 * q:6 * q + 6] - pm[q]).max() <= 2e-8 * np.abs(full).max()
    # NULL arguments
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_joint_marginals(eng.h, 2, None, 0, None))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_joint_marginal_stats(eng.h, None))
    # after PCG: refused with the solver's name; the direct solver serves again
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8)
    eng.linearize()
    assert eng.solve_gn() == 0
    with pytest.raises(hipapi.HipError, match="PCG"):
        eng.joint_marginals([act[0], act[-1]])
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.linearize()
    assert eng.solve_gn() == 0
    j = eng.joint_marginals([act[0], act[-1]])
    eng.release_marginals()   # frees the workspace; the next call allocates it again
    assert np.array_equal(eng.joint_marginals([act[0], act[-1]]), j)
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="re-linearised"):
        eng.joint_marginals([act[0], act[-1]])
    assert eng.solve_gn() == 0
    eng.joint_marginals([act[0], act[-1]])
    eng.close()


def test_distributed_solve_refused_and_replicated_served():
    sc = scene.make_scene(40, 200, 6, lm_dim=1, seed=17)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    ref = _engine(sc, 1, pa, keep=False)
    _solve(ref)
    want = ref.eng.joint_marginals([1, 30])
    ref.eng.close()
    # replicated solve on rank 0 of 2 (a no-op all-reduce hook): served
    s = _engine(sc, 1, pa, keep=False)
    s.eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 2)
    assert not s.eng.solve_is_distributed()
    _solve(s)
    assert _blk_err(s.eng.joint_marginals([1, 30]), want) < 1e-12
    s.eng.close()
    # the hooks of the distributed solve installed (no collective runs): refused, and the engine still answers
    s = _engine(sc, 1, pa, keep=False)
    s.eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 2)
    s.eng.set_collectives(lambda op, ptr, count, root: 0)
    assert s.eng.solve_is_distributed()
    with pytest.raises(hipapi.HipError, match="distributed solve"):
        s.eng.joint_marginals([1, 30])
    assert s.eng.joint_marginal_stats()["columns"] == 0
    s.eng.close()


def test_scale_configs1():
    """configs[1] (1 000 poses, n = 5 988): 64 poses spread over the trajectory (384 columns) against inv(S); the
    two-pose call costs less device time than the selected inverse of the same process."""
    sc = scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa)
    _solve(s)
    eng = s.eng
    act = np.nonzero(pa)[0]
    rows = _natural_rows(pa)
    ids = [int(p) for p in act[np.linspace(0, len(act) - 1, 64).astype(int)]]
    joint = eng.joint_marginals(ids)
    st64 = eng.joint_marginal_stats()
    assert st64["columns"] == 384
    S = eng.get_S()
    ev = np.abs(np.linalg.eigvalsh(S))   # S is symmetric: cond_2 = max |lambda| / min |lambda|
    tol = max(1e-9, 4.5 * EPS * ev.max() / ev.min())
    assert tol <= 1e-8, "scene too ill-conditioned for the check: %g" % tol
    r = _rows_of(rows, ids)
    E = np.zeros((S.shape[0], len(r)))
    E[r, np.arange(len(r))] = 1.0
    want = np.linalg.solve(S, E)[r]      # the columns of inv(S) the block needs
    err = _blk_err(joint, want)
    print("configs[1], 64 poses: err %.3g tol %.3g; %s" % (err, tol, st64))
    assert err <= tol
    assert np.array_equal(joint, joint.T)
    pat = eng.factor_tile_pattern()
    reach, prod = _plan_counts(pat, sorted({int(x) // 64 for x in r}))
    assert st64["reach_tiles"] == reach and st64["tile_products"] == 6 * prod
    # two far poses against the selected inverse
    pair = [ids[0], ids[-1]]
    eng.joint_marginals(pair)            # the workspace exists: the next call's times are the kernels' own
    j2 = eng.joint_marginals(pair)
    st2 = eng.joint_marginal_stats()
    ends = list(range(6)) + list(range(378, 384))
    assert _blk_err(j2, joint[np.ix_(ends, ends)]) <= tol
    eng.compute_marginals()
    eng.release_marginals()
    eng.compute_marginals()              # the second request, as marginals_report measures it
    ms = eng.marginal_stats()
    print("configs[1], 2 poses: solve %.3f ms + gram %.3f ms against selinv %.3f ms; products %d against %d; %s"
          % (st2["solve_ms"], st2["gram_ms"], ms["selinv_ms"], st2["tile_products"], ms["tile_products"], st2))
    assert st2["solve_ms"] + st2["gram_ms"] < ms["selinv_ms"]
    eng.close()


def test_three_lap_route():
    """The three-lap route (6 000 poses, n = 35 988: too large to download), natural order.  A far pair's joint
    block: diagonal blocks equal pose_marginals within 2 tol_route (1e-8, the bound test_marginals_gpu uses
    where S cannot be inverted on the host), the block is positive definite, the reach and the products are the
    host plan's."""
    tol_route = 1e-8
    sc = scene.make_revisit_scene(6000, 120000, 3, 40, 0.3, seed=0)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, keep=False)
    _solve(s)
    eng = s.eng
    act = np.nonzero(pa)[0]
    rows = _natural_rows(pa)
    pair = [int(act[1]), int(act[len(act) // 2])]
    joint = eng.joint_marginals(pair)
    st = eng.joint_marginal_stats()
    pat = eng.factor_tile_pattern()
    nt = pat.shape[0]
    r = _rows_of(rows, pair)
    reach, prod = _plan_counts(pat, sorted({int(x) // 64 for x in r}))
    print("three-lap route: %s" % st)
    assert st["reach_tiles"] == reach <= nt and st["tile_products"] == prod
    assert np.all(np.isfinite(joint)) and np.array_equal(joint, joint.T)
    np.linalg.cholesky(joint)
    pm = eng.pose_marginals(pair)
    ms = eng.marginal_stats()
    scale = np.abs(joint).max()
    for i in range(2):
        d = np.abs(joint[6 * i:6 * i + 6, 6 * i:6 * i + 6] - pm[i]).max() / scale
        print("three-lap route: pose %d diagonal block differs by %.3g of the joint's maximum" % (pair[i], d))
        assert d <= 2 * tol_route
    print("three-lap route: joint %.3f + %.3f ms against selinv %.3f ms" % (st["solve_ms"], st["gram_ms"], ms["selinv_ms"]))
    eng.close()
