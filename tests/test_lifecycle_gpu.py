"""ba_hip_finalize drops what the engine held of the system before it (lifecycle.h, DESIGN.md "What the engine holds
and what drops it"): after solve_gn -> getters -> the same scene uploaded again -> finalize, every reader of the kept
factor refuses with the usual "needs the factor of the last ba_hip_solve_gn" message instead of reading the factor,
the selected inverse and its slot table of a system that is gone; after a new linearise and solve_gn the results are
those of the first round.  The second system has the size of the first on purpose: a stale read stays inside its
buffers, the test never needs an out-of-bounds access to fail.  Tolerance: max(1e-9, 4.5 eps cond(S)) of
leverage_cases.tolerance, covariances in correlation units (joint_state_cases.corr_err), hat blocks absolutely."""
import numpy as np
import pytest

from ba_amd import hipapi, scene
from helpers import _add_pose_pose
from joint_state_cases import corr_err
import leverage_cases as lc

pytestmark = pytest.mark.gpu

P, L = 14, 60
REFUSED = "needs the factor of the last ba_hip_solve_gn \\(none yet, or the system was re-linearised since\\)"


def _scene():
    """LmSize 1, 14 poses of which the first two are fixed (72 pose rows: two tiles), 60 landmarks seen by 3 to 5
    poses each (the reference pose and 2 to 4 accepted residuals)"""
    sc = scene.make_scene(P, L, 4, lm_dim=1, seed=11, anchors=(0, 1))
    pa = np.ones(P, dtype=np.uint8)
    pa[:2] = 0
    k = np.arange(len(sc.obs_pose)) % 5          # 0: the reference observation (rejected), 1 .. 4 accepted
    keep = (k >= 1) & (k <= 2 + sc.obs_lm % 3)
    return sc, pa, (sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])


def _upload(eng, sc, pa, obs, pose_pose):
    """the whole problem into the engine, finalized (natural order)"""
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(*obs)
    if pose_pose:
        _add_pose_pose(eng, sc, P)
    eng.set_pose_ordering(hipapi.ORDER_NATURAL)
    eng.finalize()


def _solve(eng):
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(P, dtype=np.uint16))
    eng.linearize()
    assert eng.solve_gn() == 0


def _engine():
    eng = hipapi.Engine(1, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.keep_reduced_system = 1
    eng.set_options(o)
    return eng


def test_refinalize_drops_the_kept_factor():
    sc, pa, obs = _scene()
    nres = len(obs[1])
    assert set(np.bincount(obs[2], minlength=L)) == {2, 3, 4}
    lev_ids = [0, 7, nres // 2, nres - 1]
    getters = {
        "pose": lambda e: e.pose_marginals([2, 9]),
        "joint": lambda e: e.joint_marginals([3, 11]),
        "joint state": lambda e: e.joint_state_marginals([2, 9], [3, 40]),
        "leverages": lambda e: e.projection_leverages(lev_ids),
    }
    eng = _engine()
    _upload(eng, sc, pa, obs, False)
    _solve(eng)
    S = eng.get_S()
    assert S.shape == (72, 72)
    tol = lc.tolerance(S)
    first = {k: g(eng) for k, g in getters.items()}
    assert eng.marginal_stats()["store_tiles"] > 1   # (the slot table of the selected inverse is not trivial)
    eng.check_solve()

    _upload(eng, sc, pa, obs, False)   # the same system again: finalize re-allocates nothing
    for name, g in getters.items():
        with pytest.raises(hipapi.HipError, match=REFUSED):
            g(eng)
    with pytest.raises(hipapi.HipError, match="ba_hip_check_solve needs keep_reduced_system and a finished ba_hip_solve_gn"):
        eng.check_solve()
    # ba_hip_get_S takes its no-factor branch: it reads A (where the old factor still lies), not the kept copy of S
    assert not np.array_equal(eng.get_S(), S)

    _solve(eng)
    second = {k: g(eng) for k, g in getters.items()}
    errs = {
        "pose": max(corr_err(b, a) for a, b in zip(first["pose"], second["pose"])),
        "joint": corr_err(second["joint"], first["joint"]),
        "joint state": corr_err(second["joint state"], first["joint state"]),
        "leverages": float(np.abs(second["leverages"] - first["leverages"]).max()),
    }
    print("second round against the first: %s, tol %.3g, cond(S) %.3g" % (errs, tol, np.linalg.cond(S)))
    for name, err in errs.items():
        assert err <= tol, name
    assert np.abs(eng.get_S() - S).max() <= tol * np.abs(S).max()
    eng.close()


def test_refinalize_refuses_pose_pose_leverages():
    sc, pa, obs = _scene()
    eng = _engine()
    _upload(eng, sc, pa, obs, True)
    _solve(eng)
    cov, _, lev = eng.pose_pose_leverages(hipapi.RES_BINARY)
    assert np.all(np.isfinite(cov)) and lev[0] == 0 and np.all(lev[1:] > 0)   # (residual 0 joins the two fixed poses)
    _upload(eng, sc, pa, obs, True)
    for kind in (hipapi.RES_UNARY, hipapi.RES_BINARY):
        with pytest.raises(hipapi.HipError, match="ba_hip_get_pose_pose_leverages: " + REFUSED):
            eng.pose_pose_leverages(kind)
    _solve(eng)
    cov2, _, lev2 = eng.pose_pose_leverages(hipapi.RES_BINARY)
    assert np.abs(lev2 - lev).max() <= lc.tolerance(eng.get_S())
    eng.close()
