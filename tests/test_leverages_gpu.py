"""Leverages of projection residuals on the MI355X (ba_hip_get_projection_leverages, k_lever.hip): the 2 x 2 hat
blocks against the diagonal blocks of Q Q^T (thin QR of the dense whitened Jacobian, no inverse involved) and
against J_a inv(H_full) J_a^T with H_full assembled from the engine's Jacobians and its kept S.  Tolerance per block:
max(1e-9, 4.5 eps cond(S)), absolute since |H| <= 1; every scene must keep it <= 1e-8."""
import numpy as np
import pytest

from ba_amd import hipapi, scene
import leverage_cases as lc
import track_cases as tc

pytestmark = pytest.mark.gpu


def _fixed(sc, more=2):
    """the anchors and `more` further poses inactive"""
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    free = [p for p in range(sc.num_poses) if pa[p]]
    pa[free[len(free) // 3::len(free) // 3][:more]] = 0
    assert int(pa.sum()) == sc.num_poses - len(set(sc.anchor_poses)) - more
    return pa


def _err(got, want):
    return np.abs(got - want).max()


def _check_blocks(got):
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, np.transpose(got, (0, 2, 1))), "not bitwise symmetric"


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("dims", [(12, 60, 4), (83, 500, 6)])
def test_all_residuals_against_qr_and_full_system(dims, lm_dim):
    """Every residual against both references; sum of the traces = unknowns.  The larger scene has 79 active poses:
    474 rows, no multiple of 64, pose blocks straddle tiles."""
    sc = scene.make_scene(*dims, lm_dim=lm_dim, seed=11)
    s = lc.engine(sc, lm_dim, _fixed(sc))
    lc.solve(s)
    S = s.eng.get_S()
    if dims[0] == 83:
        assert S.shape[0] % 64 != 0
    tol = lc.tolerance(S)
    got = s.eng.projection_leverages()
    _check_blocks(got)
    J, n = lc.engine_jacobian(s)
    assert n == S.shape[0]
    ids = list(range(len(s.obs_pose)))
    e_qr, e_full = _err(got, lc.qr_blocks(J)), _err(got, lc.hfull_form(s, S, J, ids))
    tr, unknowns = np.trace(got, axis1=1, axis2=2).sum(), lc.unknowns_seen(s)
    print("lm%d %s: |H - QR| %.3g, |H - full| %.3g, tol %.3g, cond(S) %.3g, sum tr %.10g of %d" %
          (lm_dim, dims, e_qr, e_full, tol, np.linalg.cond(S), tr, unknowns))
    assert e_qr <= tol and e_full <= tol
    assert abs(tr - unknowns) <= 1e-7 * unknowns
    st = s.eng.leverage_stats()
    assert st["residuals"] == len(ids) and st["landmarks"] == sc.num_landmarks and st["device_ms"] > 0
    assert st["block_reads"] >= len(ids)
    s.eng.close()


def test_pose_pose_terms_and_masks():
    """Unary priors, odometry and three masked translation parameters of the first active pose: the hat blocks of
    the projection residuals inside the larger system, against the full-system form."""
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    pa = _fixed(sc)
    masks = np.zeros(sc.num_poses, dtype=np.uint16)
    masks[int(np.nonzero(pa)[0][0])] = 0x7
    s = lc.engine(sc, 1, pa, pose_pose=True, masks=masks)
    lc.solve(s)
    S = s.eng.get_S()
    tol = lc.tolerance(S)
    got = s.eng.projection_leverages()
    _check_blocks(got)
    J, _ = lc.engine_jacobian(s)
    r0 = lc.natural_rows(pa)[int(np.nonzero(pa)[0][0])]
    assert np.all(J[:, r0:r0 + 3] == 0) and np.all(np.diag(S)[r0:r0 + 3] == 1e6)
    err = _err(got, lc.hfull_form(s, S, J, list(range(len(got)))))
    print("pose-pose + masks: |H - full| %.3g, tol %.3g, cond(S) %.3g" % (err, tol, np.linalg.cond(S)))
    assert err <= tol
    ev = np.linalg.eigvalsh(got)
    assert ev.min() >= -tol and ev.max() <= 1 + tol
    s.eng.close()


def test_inactive_landmarks():
    """Three inactive landmarks: their residuals keep A Sigma A^T only (B and the Schur part drop out)."""
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    la[[4, 17, 41]] = 0
    s = lc.engine(sc, 1, _fixed(sc), lm_active=la)
    lc.solve(s)
    S = s.eng.get_S()
    tol = lc.tolerance(S)
    got = s.eng.projection_leverages()
    _check_blocks(got)
    J, n = lc.engine_jacobian(s)
    ids = list(range(len(got)))
    e_full, e_qr = _err(got, lc.hfull_form(s, S, J, ids)), _err(got, lc.qr_blocks(J))
    print("inactive landmarks: |H - full| %.3g, |H - QR| %.3g, tol %.3g" % (e_full, e_qr, tol))
    assert e_full <= tol and e_qr <= tol
    off = np.nonzero(~la[s.obs_lm].astype(bool))[0]
    assert len(off) == 12
    Sig = np.linalg.inv(S)
    for a in off:
        A = J[2 * a:2 * a + 2, :n]
        assert _err(got[a], A @ Sig @ A.T) <= tol
    tr = np.trace(got, axis1=1, axis2=2).sum()
    assert abs(tr - lc.unknowns_seen(s)) <= 1e-7 * lc.unknowns_seen(s)
    s.eng.close()


def test_reference_pose_observations_and_zero_weights():
    """LmSize 1 with every landmark's observation from its own reference pose kept as a residual: it carries no pose
    block (the listing rule of lm_entry: H_aa = B Sigma_ll B^T, which is zero up to rounding here, since the pixel in
    the reference frame does not depend on the inverse depth), and it is no incidence of the landmark.  Five
    residuals of weight zero read exactly zero."""
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    w = np.ones(len(sc.obs_pose))
    zero = [3, 50, 51, 160, 299]
    w[zero] = 0.0
    s = lc.engine(sc, 1, _fixed(sc), obs=(sc.obs_z, sc.obs_pose, sc.obs_lm), weight=w)
    own = np.nonzero(s.obs_pose == sc.lm_ref_pose[s.obs_lm])[0]
    assert len(own) == sc.num_landmarks and set(zero) & set(own.tolist())
    lc.solve(s)
    S = s.eng.get_S()
    tol = lc.tolerance(S)
    got = s.eng.projection_leverages()
    _check_blocks(got)
    J, n = lc.engine_jacobian(s)
    assert np.all(J[np.r_[2 * own, 2 * own + 1], :n] == 0)
    ids = list(range(len(got)))
    e_full, e_qr = _err(got, lc.hfull_form(s, S, J, ids)), _err(got, lc.qr_blocks(J))
    print("reference-pose observations: |H - full| %.3g, |H - QR| %.3g, tol %.3g" % (e_full, e_qr, tol))
    assert e_full <= tol and e_qr <= tol
    assert np.all(got[zero] == 0.0)
    # (seen from its own reference frame the pixel does not depend on the inverse depth either: dz_dlm = 0)
    assert np.abs(got[own]).max() <= tol and np.abs(np.delete(got, own, 0)).max() > 0.1
    assert np.array_equal(s.eng.projection_leverages(zero + [int(own[7])]), got[zero + [int(own[7])]])
    s.eng.close()


@pytest.mark.parametrize("kind", ["tvs", "calib4"])
def test_calibration(kind):
    """LmSize 1 with calibration columns behind the poses: DoTvs (six) and CalibSize 4; the scenes, priors and
    odometry of the calibration tests of tests/test_marginals_gpu.py (the rows straddle a tile boundary)."""
    if kind == "tvs":
        sc = scene.make_scene(44, 300, 6, lm_dim=1, seed=12)
        pa = np.ones(sc.num_poses, dtype=np.uint8)
        pa[sc.anchor_poses] = 0
        s = lc.engine(sc, 1, pa, tvs=True, pose_pose=True)
    else:
        sc = scene.make_scene(25, 300, 6, lm_dim=1, seed=18)
        pa = np.ones(sc.num_poses, dtype=np.uint8)
        pa[sc.anchor_poses] = 0
        pa[::10] = 0
        s = lc.engine(sc, 1, pa, calib=4, pose_pose=True)
    lc.solve(s)
    S = s.eng.get_S()
    n, K = S.shape[0], s.K
    assert (n - K) // 64 != (n - 1) // 64, "calibration rows do not straddle a tile"
    tol = lc.tolerance(S)
    got = s.eng.projection_leverages()
    _check_blocks(got)
    J, nn = lc.engine_jacobian(s)
    assert nn == n and np.abs(J[:, n - K:n]).max() > 0
    err = _err(got, lc.hfull_form(s, S, J, list(range(len(got)))))
    print("%s: |H - full| %.3g, tol %.3g, cond(S) %.3g" % (kind, err, tol, np.linalg.cond(S)))
    assert err <= tol
    ev = np.linalg.eigvalsh(got)
    assert ev.min() >= -tol and ev.max() <= 1 + tol
    s.eng.close()


def test_calibration_with_long_tracks():
    """DoTvs on `long_tracks` of tests/track_cases.py (65 to 700 observations; the banked trajectory of the calibration
    tests, every third pose fixed, priors and odometry): the calibration incidence's slot of the stage together with
    the two-sweep path.  Every residual of the long landmarks against the full-system form, and by id bit for bit."""
    lengths = np.asarray(tc.cases(1)["long_tracks"])
    sc, z, pose, lm = tc.build(1, lengths, roll_amp=0.6)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[::3] = 0
    s = lc.engine(sc, 1, pa, tvs=True, pose_pose=True, obs=(z, pose, lm))
    lc.solve(s)
    S = s.eng.get_S()
    tol = lc.tolerance(S)
    got = s.eng.projection_leverages()
    _check_blocks(got)
    ids = [int(a) for a in np.nonzero(np.isin(s.obs_lm, tc.long_ids(lengths)))[0]]
    assert len(ids) == 65 + 127 + 128 + 129 + 200 + 700
    J, n = lc.engine_jacobian(s)
    assert np.abs(J[:, n - 6:n]).max() > 0
    err = _err(got[ids], lc.hfull_form(s, S, J, ids))
    ev = np.linalg.eigvalsh(got)
    print("tvs + long tracks: |H - full| %.3g, tol %.3g, cond(S) %.3g, eig in [%.3g, %.12g]" %
          (err, tol, np.linalg.cond(S), ev.min(), ev.max()))
    assert err <= tol
    assert ev.min() >= -tol and ev.max() <= 1 + tol
    assert np.array_equal(s.eng.projection_leverages(ids[::-1]), got[ids[::-1]])
    assert s.eng.leverage_stats()["landmarks"] == 6
    s.eng.close()


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_track_length_edges(lm_dim):
    """`mixed` of tests/track_cases.py: tracks of 1 (LmSize 3: 2), 64, 65, 128, 129, 700 observations, empty
    landmarks, several observations of a landmark from one pose.  Every residual of the long landmarks (more than 64:
    the two-sweep path), of two landmarks with exactly 64 and of one with the shortest track against the full-system
    form; every block in [0, 1]; the rest by the sum of the traces."""
    lengths = np.asarray(tc.cases(lm_dim)["mixed"])
    sc, z, pose, lm = tc.build(lm_dim, lengths)
    s = lc.engine(sc, lm_dim, tc.anchored(sc), obs=(z, pose, lm))
    lc.solve(s)
    S = s.eng.get_S()
    tol = lc.tolerance(S)
    got = s.eng.projection_leverages()
    _check_blocks(got)
    short = 1 if lm_dim == 1 else 2
    lms = list(tc.long_ids(lengths)) + list(np.nonzero(lengths == 64)[0][:2]) + [int(np.nonzero(lengths == short)[0][0])]
    assert {65, 128, 129, 700} <= set(lengths[lms].tolist())
    ids = [int(a) for a in np.nonzero(np.isin(s.obs_lm, lms))[0]]
    assert len(ids) == int(lengths[lms].sum())
    dup = sum(len(p) - len(set(p)) for p in (s.obs_pose[s.obs_lm == l].tolist() for l in lms))
    assert dup > 0, "no landmark observed twice from one pose"
    J, _ = lc.engine_jacobian(s)
    err = _err(got[ids], lc.hfull_form(s, S, J, ids))
    ev = np.linalg.eigvalsh(got)
    tr, unknowns = np.trace(got, axis1=1, axis2=2).sum(), lc.unknowns_seen(s)
    print("mixed lm%d: %d residuals checked, |H - full| %.3g, tol %.3g, cond(S) %.3g, eig in [%.3g, %.12g], "
          "sum tr %.10g of %d" % (lm_dim, len(ids), err, tol, np.linalg.cond(S), ev.min(), ev.max(), tr, unknowns))
    assert err <= tol
    assert ev.min() >= -tol and ev.max() <= 1 + tol
    assert abs(tr - unknowns) <= 1e-7 * unknowns
    st = s.eng.leverage_stats()
    assert st["landmarks"] == int((lengths > 0).sum()) and st["residuals"] == len(got)
    s.eng.close()


def test_by_id_equals_all_bitwise_and_orderings_agree():
    """A shuffled subset of ids with repeats equals the all-residuals output bit for bit (a long track included), two
    calls give the same bits, and BA_HIP_ORDER_AUTO changes nothing beyond the tolerance — nor does a reversed pose
    order (ORDER_USER), which moves every pose block whatever AUTO chooses on a scene of this size."""
    lengths = np.asarray(tc.cases(1)["around_64"])
    sc, z, pose, lm = tc.build(1, lengths)
    pa = tc.anchored(sc)
    res = []
    rev = np.arange(int(pa.sum()), dtype=np.uint32)[::-1]
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO, hipapi.ORDER_USER):
        s = lc.engine(sc, 1, pa, mode=mode, obs=(z, pose, lm), perm=rev if mode == hipapi.ORDER_USER else None)
        if mode == hipapi.ORDER_USER:
            assert np.array_equal(s.eng.get_pose_ordering()[0], rev)
        lc.solve(s)
        every = s.eng.projection_leverages()
        assert np.array_equal(every, s.eng.projection_leverages())
        rng = np.random.default_rng(5)
        long_res = np.nonzero(np.isin(s.obs_lm, tc.long_ids(lengths)))[0]
        ids = np.concatenate([rng.choice(len(every), 200, replace=False), long_res[::3], [7, 7, 7]])
        ids = rng.permutation(ids)
        assert len(set(ids.tolist())) < len(ids)
        per = s.eng.projection_leverages(ids)
        assert np.array_equal(per, every[ids])
        assert np.array_equal(per, s.eng.projection_leverages(ids))
        assert s.eng.leverage_stats()["residuals"] == len(ids)
        res.append((every, lc.tolerance(s.eng.get_S())))
        s.eng.close()
    (nat, tol), (auto, _), (user, _) = res
    print("natural against AUTO: %.3g, against a reversed order: %.3g, tol %.3g" % (_err(auto, nat), _err(user, nat), tol))
    assert _err(auto, nat) <= tol and _err(user, nat) <= tol


def test_refusals():
    """Each refusal carries a message, the engine stays usable after it, and a request after
    ba_hip_release_marginals is served again."""
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    pa = _fixed(sc)
    s = lc.engine(sc, 1, pa)
    eng = s.eng
    with pytest.raises(hipapi.HipError, match="ba_hip_get_projection_leverages: needs the factor"):
        eng.projection_leverages()
    lc.solve(s)
    want = eng.projection_leverages()
    O = len(want)
    with pytest.raises(hipapi.HipError, match="id %d is not a projection residual" % O):
        eng.projection_leverages([0, O])
    with pytest.raises(hipapi.HipError, match="n must be the projection residual count"):
        eng.projection_leverages(None, count=O - 1)
    assert np.array_equal(eng.projection_leverages([3]), want[[3]])
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="re-linearised"):
        eng.projection_leverages([3])
    assert eng.solve_gn() == 0
    assert np.array_equal(eng.projection_leverages(), want)
    eng.set_reduced_solver(hipapi.SOLVER_PCG)
    eng.linearize()
    assert eng.solve_gn() == 0
    with pytest.raises(hipapi.HipError, match="PCG"):
        eng.projection_leverages([3])
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    lc.solve(s)
    assert np.array_equal(eng.projection_leverages(), want)
    eng.release_marginals()
    assert np.array_equal(eng.projection_leverages([5, 2]), want[[5, 2]])
    eng.close()
    # an all-reduce hook makes the engine sharded: each rank holds one landmark shard
    s = lc.engine(sc, 1, pa)
    s.eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 2)
    lc.solve(s)
    with pytest.raises(hipapi.HipError, match="sharded"):
        s.eng.projection_leverages([0])
    s.eng.pose_marginals([int(np.nonzero(pa)[0][0])])
    s.eng.close()
    # LmSize 0: no projection residuals at all
    eng = hipapi.Engine(0, 6)
    with pytest.raises(hipapi.HipError, match="LmSize 0"):
        eng.projection_leverages([0])
    eng.close()


def test_through_the_class():
    """ba::BundleAdjuster::GetProjectionLeverage / GetProjectionRedundancy (adjuster.py -> ba_capi): the values of
    the C-ABI for the caller's residual ids; the id of a rejected residual is refused."""
    from ba_amd import adjuster
    from helpers import fill
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    h = adjuster.BundleAdjuster(1, 6)
    o = adjuster.default_options()
    o.use_dogleg = 0
    h.Init(o)
    ids = np.asarray(fill(h, sc, active=_fixed(sc)), dtype=np.uint32)
    rejected = ids == 0xFFFFFFFF
    assert rejected.sum() == sc.num_landmarks and h.GetNumProjResiduals() == int((~rejected).sum())
    h.Solve(1)
    assert adjuster.RESULT_NAMES[h.summary().result] not in ("FactorizationError", "SolverError")
    pick = ids[~rejected][[0, 57, 200]]
    want = h.engine().projection_leverages(pick)
    for q, a in enumerate(pick):
        got = h.projection_leverage(a)
        assert np.array_equal(got, want[q])
        assert h.projection_redundancy(a) == 2.0 - (want[q][0, 0] + want[q][1, 1])
        assert 0.0 < h.projection_redundancy(a) < 2.0
    with pytest.raises(RuntimeError, match="unavailable"):
        h.projection_leverage(0xFFFFFFFF)
    with pytest.raises(RuntimeError, match="unavailable"):
        h.projection_redundancy(h.GetNumProjResiduals())
