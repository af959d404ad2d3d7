"""Multi-RHS solves with the kept factor on the MI355X (ba_hip_factor_solve, k_factorsolve.hip): X = S^-1 B for
the caller's columns.  The test tap ba_hip_tile_factor_solve runs the cases of factor_solve_cases.py (patterns and
pivot signs that no scene produces) against numpy.linalg.solve within both bounds of that module and against the
host restatement; scenes check the public call against the Gauss-Newton step, numpy.linalg.solve on the kept S
and the columns of inv(S) that joint_marginals returns, under every pose ordering, and what the call must refuse
and leave alone.  Forward tolerance: max(1e-9, 4.5 eps cond(S)) relative to the largest entry of the reference
(DESIGN.md section 8)."""
import numpy as np
import pytest

import factor_solve_cases as fc
from ba_amd import hipapi, scene
from test_factor_solve_plan import hc, host_solve  # noqa: F401  (hc is a fixture)
from test_marginals_gpu import _engine, _natural_rows, _sym, _tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tap():
    eng = hipapi.Engine(1, 6)
    yield eng
    eng.close()


@pytest.mark.parametrize("name,m,kind", fc.instances())
def test_tile_cases(tap, hc, name, m, kind):  # noqa: F811
    c, S, lower, tmap = fc.case(name)
    B = fc.rhs(name, m, kind)
    X, rc = tap.tile_factor_solve(lower, B, tmap)
    assert rc == 0
    rr, fe = fc.check_solution(name, m, kind, X)
    Xh = host_solve(hc, S, B, tmap)[0]
    fh = fc.forward_err(X, Xh)
    print("%s m=%d %s: residual %.3g n eps, forward %.3g, against the host %.3g (tol %.3g)"
          % (name, m, kind, rr, fe, fh, fc.forward_tol(name)))
    assert fh <= fc.forward_tol(name)
    st = tap.factor_solve_stats()
    fl, bl, fprod, bprod, _ = fc.mirror_plan(c.nzL, m)
    assert st["columns"] == m and st["tiles"] == c.nt
    assert st["forward_levels"] == fl.max() + 1 and st["backward_levels"] == bl.max() + 1
    assert st["tile_products"] == fprod + bprod


def test_tile_case_twice_same_bits(tap):
    c, S, lower, tmap = fc.case("dense6neg")
    B = fc.rhs("dense6neg", 130, "random")
    X1, _ = tap.tile_factor_solve(lower, B, tmap)
    tap.tile_factor_solve(fc.case("two")[2], fc.rhs("two", 1, "random"))   # a request of another shape in between
    X2, _ = tap.tile_factor_solve(lower, B, tmap)
    assert np.array_equal(X1, X2)


# ---- scenes ------------------------------------------------------------------------------------------------
def _solve_keep_rhs(s):
    """one Gauss-Newton iteration left factorised (_solve of test_marginals_gpu), the right-hand side read first"""
    s.eng.linearize()
    b = s.eng.get_rhs()[0]
    assert s.eng.solve_gn() == 0
    return b


def _scene_checks(s, b, ids, calibration=False):
    eng = s.eng
    S = _sym(eng.get_S())
    n = S.shape[0]
    assert n == eng.num_pose_params() + eng.num_calib_params()
    tol = _tol(S)
    # the step: one column
    x1 = eng.factor_solve(b)
    assert x1.shape == (n,)
    delta = eng.get_delta_gn()[0]
    e1 = fc.forward_err(x1, delta)
    # 65 random columns
    B = np.random.default_rng(5).standard_normal((n, 65))
    X = eng.factor_solve(B)
    want = np.linalg.solve(S, B)
    e65 = fc.forward_err(X, want)
    rr = fc.residual_ratio(S, B, X)
    st = eng.factor_solve_stats()
    print("n = %d: step err %.3g, 65 columns err %.3g (tol %.3g), residual %.3g n eps; %s" % (n, e1, e65, tol, rr, st))
    assert e1 <= tol and e65 <= tol and rr <= 1.0
    assert st["columns"] == 65 and st["tiles"] == (n + 63) // 64 and st["forward_ms"] > 0 and st["backward_ms"] > 0
    assert np.array_equal(eng.factor_solve(B), X)
    # unit columns: the columns of inv(S) that joint_marginals returns
    rows = _natural_rows(s.pa)
    r = [rows[p] + x for p in ids for x in range(6)] + (list(range(n - s.K, n)) if calibration else [])
    E = np.zeros((n, len(r)))
    E[r, np.arange(len(r))] = 1.0
    cols = eng.factor_solve(E)
    joint = eng.joint_marginals(ids, include_calibration=calibration)
    assert np.abs(cols[r] - joint).max() <= 2 * tol * np.abs(joint).max()
    assert fc.forward_err(cols, np.linalg.solve(S, E)) <= tol
    return X


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_fixed_poses_and_pose_pose_terms(lm_dim):
    sc = scene.make_scene(83, 500, 6, lm_dim=lm_dim, seed=11)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[[9, 40]] = 0
    s = _engine(sc, lm_dim, pa, pose_pose=True)
    b = _solve_keep_rhs(s)
    assert s.eng.num_pose_params() % 64 != 0
    act = [int(p) for p in np.nonzero(pa)[0]]
    _scene_checks(s, b, [act[-1], act[0], act[17]])
    s.eng.close()


def test_orderings(monkeypatch):
    """make_scene(400, 1200, 6): natural order, ORDER_AUTO and a caller's permutation that is not tile aligned (a
    rotation by 5 poses = 30 rows) give the solution in the caller's rows."""
    sc = scene.make_scene(400, 1200, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    act = [int(p) for p in np.nonzero(pa)[0]]
    nact = len(act)
    perm = ((np.arange(nact) + 5) % nact).astype(np.uint32)
    res = {}
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO, hipapi.ORDER_USER):
        with monkeypatch.context() as mp:
            if mode == hipapi.ORDER_USER:   # _engine sets the mode; the permutation goes with it
                plain = hipapi.Engine.set_pose_ordering
                mp.setattr(hipapi.Engine, "set_pose_ordering",
                           lambda self, md: (plain(self, md), self.set_pose_permutation(perm))[0])
            s = _engine(sc, 1, pa, mode=mode)
        b = _solve_keep_rhs(s)
        if mode == hipapi.ORDER_USER:
            assert np.array_equal(s.eng.get_pose_ordering()[0], perm)
        res[mode] = _scene_checks(s, b, [act[1], act[-1], act[nact // 2]])
        tol = _tol(_sym(s.eng.get_S()))
        s.eng.close()
    for mode in (hipapi.ORDER_AUTO, hipapi.ORDER_USER):
        assert fc.forward_err(res[mode], res[hipapi.ORDER_NATURAL]) <= tol


def test_calibration_rows_with_tvs():
    """DoTvs: the six calibration rows come last and straddle a tile."""
    sc = scene.make_scene(44, 300, 6, lm_dim=1, seed=12)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, tvs=True, pose_pose=True)
    b = _solve_keep_rhs(s)
    n = s.eng.num_pose_params() + s.eng.num_calib_params()
    assert s.eng.num_calib_params() == 6 and (n - 6) // 64 != (n - 1) // 64
    act = [int(p) for p in np.nonzero(pa)[0]]
    _scene_checks(s, b, [act[2], act[-1]], calibration=True)
    s.eng.close()


def test_refusals():
    sc = scene.make_scene(40, 200, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, keep=False)
    eng = s.eng
    n = eng.num_pose_params()
    B = np.random.default_rng(1).standard_normal((n, 3))
    with pytest.raises(hipapi.HipError, match="ba_hip_factor_solve: needs the factor of the last ba_hip_solve_gn"):
        eng.factor_solve(B)
    assert eng.factor_solve_stats()["columns"] == 0
    _solve_keep_rhs(s)
    good = eng.factor_solve(B)
    with pytest.raises(hipapi.HipError, match="m == 0"):
        eng.factor_solve(np.zeros((n, 0)))
    with pytest.raises(hipapi.HipError, match="513 columns requested, the limit is BA_HIP_FACTOR_SOLVE_MAX_COLUMNS \\(512\\)"):
        eng.factor_solve(np.zeros((n, 513)))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_factor_solve(eng.h, 3, None, None))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_factor_solve_stats(eng.h, None))
    assert np.array_equal(eng.factor_solve(B), good)
    full = eng.factor_solve(np.ones((n, 512)))   # the limit itself: eight column blocks
    assert np.array_equal(full[:, 0], full[:, 511]) and np.all(np.isfinite(full))
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="re-linearised"):
        eng.factor_solve(B)
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8)
    assert eng.solve_gn() == 0
    with pytest.raises(hipapi.HipError, match="PCG"):
        eng.factor_solve(B)
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.linearize()
    assert eng.solve_gn() == 0
    assert np.array_equal(eng.factor_solve(B), good)
    # a stand-alone solve replaces the kept factor
    eng.tile_factor_solve(fc.case("two")[2], fc.rhs("two", 1, "random"))
    with pytest.raises(hipapi.HipError, match="stand-alone solve"):
        eng.factor_solve(B)
    eng.close()


def test_non_interference_and_release():
    """A run that solves with the factor between two Gauss-Newton solves gives bitwise the steps, pose_marginals,
    joint_marginals and the counts of marginal_stats of a run that never does; marginal_stats does not move across
    the call; release_marginals gives the workspace back."""
    sc = scene.make_scene(70, 300, 6, lm_dim=1, seed=14)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    act = [int(p) for p in np.nonzero(pa)[0]]
    ids = [act[-1], act[0], act[20]]
    outs = []
    for ask in (False, True):
        s = _engine(sc, 1, pa, tvs=True)
        eng = s.eng
        rec = []
        for it in range(2):
            eng.linearize()
            assert eng.solve_gn() == 0
            if ask:
                n = eng.num_pose_params() + eng.num_calib_params()
                B = np.random.default_rng(it).standard_normal((n, 70))
                if it == 1:
                    eng.pose_marginals(ids)   # the Sigma store exists and is valid: it must stay so
                before, jbefore = eng.marginal_stats(), eng.joint_marginal_stats()
                live = hipapi.device_bytes_live()
                x1 = eng.factor_solve(B)
                assert hipapi.device_bytes_live() > live or it == 1   # (the second solve finds the workspace)
                assert np.array_equal(eng.factor_solve(B), x1)
                assert eng.marginal_stats() == before and eng.joint_marginal_stats() == jbefore
                if it == 0:
                    assert before["selinv_ms"] == 0 and before["store_bytes"] == 0
                    eng.release_marginals()
                    assert hipapi.device_bytes_live() == live
                    assert np.array_equal(eng.factor_solve(B), x1)   # allocated again
            rec.append(eng.pose_marginals(ids))
            rec.append(eng.joint_marginals(ids, include_calibration=True))
            ms = eng.marginal_stats()
            rec.append(np.array([ms[k] for k in sorted(ms) if not k.endswith("_ms")], dtype=np.float64))
            rec += list(eng.get_delta_gn())
            eng.compose_step(0.0, 1.0)
            rec += list(eng.get_step())
            eng.apply_step()
        eng.end_solve()
        rec.append(eng.get_poses(sc.num_poses)[0])
        outs.append(rec)
        eng.close()
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
