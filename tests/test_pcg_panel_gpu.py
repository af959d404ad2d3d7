"""The panel PCG on the MI355X (ba_hip_pcg_panel_solve_system, ba_hip_get_joint_marginals_pcg; k_pcg_panel.hip).
The test tap ba_hip_pcg_panel_solve runs the cases of tests/pcg_panel_cases.py against numpy within the two bounds of
pcg_cases and against the host restatement (equal iteration counts; X within the forward bound — not bitwise, the
order inside an MFMA's group of four k is not restated); a second call, a column alone, permuted columns and a
panel widened across the 64-column boundary return the same bits; a column that breaks down leaves its neighbours'
bits alone.  Scenes check the public calls after a PCG solve_gn under every pose ordering and with calibration
rows against numpy on ba_hip_get_S and against the direct solver's joint marginals, what the calls refuse, that they
leave the engine's results and its next iteration alone, and that the work space comes back."""
import numpy as np
import pytest

import pcg_cases as pc
import pcg_panel_cases as pp
from ba_amd import hipapi, scene
from test_marginals_gpu import _engine, _natural_rows, _sym
from test_pcg_panel_plan import hc, panel as host_panel  # noqa: F401  (hc is a fixture)

pytestmark = pytest.mark.gpu

SYSTEMS = pp.systems()
EPS = pc.EPS


@pytest.fixture(scope="module")
def tap():
    eng = hipapi.Engine(1, 6)
    yield eng
    eng.close()


# ---- the tap on the shared cases --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_tap_on_the_shared_cases(tap, hc, name):  # noqa: F811
    S, D, K = SYSTEMS[name]
    n = S.shape[0]
    cond = pp.cond_of(name)
    for m in pp.WIDTHS:
        B = pp.columns(name, S, m)
        XS = np.linalg.solve(S, B)
        for tol in pp.TOLS:
            # as test_pcg_gpu: the tap takes one block size, the border of K rows falls into blocks of D like the rest
            X, rc, st = tap.pcg_panel_solve(np.tril(S), B, D, tol, max_iterations=n)
            col = tap.pcg_panel_columns(m)
            assert rc == 0 and st["columns"] == m and st["column_blocks"] == (m + 63) // 64, st
            assert st["converged"] == m and st["capped"] == 0 and st["broken_down"] == 0, st
            assert np.all(col["converged"] == 1) and np.all(col["breakdown"] == 0)
            worst = pp.assert_panel_bounds(S, cond, B, X, tol, range(m))
            Xh, rch, sh = host_panel(hc, S, B, D, 0, tol, max_it=n)
            assert rch == 0 and np.array_equal(col["iterations"], sh["iterations"]), (m, tol, col["iterations"], sh["iterations"])
            assert st["passes"] >= sh["passes"] and st["tile_products_per_pass"] == sh["sources"] * ((m + 63) // 64)
            bound = cond * tol + 4.5 * EPS * cond
            for j in range(m):
                ref = np.linalg.norm(XS[:, j])
                assert np.linalg.norm(X[:, j] - Xh[:, j]) <= bound * ref, (m, tol, j)
            if m > 2:
                assert np.all(X[:, 2] == 0.0) and col["iterations"][2] == 0 and col["converged"][2] == 1
            if name == "composite" and m >= 2:
                assert col["iterations"][0] == 1 and col["iterations"][1] >= 40
            print("%s m=%d tol %.0e: %d passes, iterations %d..%d, residual %.2e, forward %.2e, host difference %.2e, %.3f ms"
                  % (name, m, tol, st["passes"], col["iterations"].min(), col["iterations"].max(), worst[0], worst[1],
                     np.abs(X - Xh).max(), st["solve_ms"]))


@pytest.mark.parametrize("name", ["composite", "chain_D9", "arrow_straddling_border"])
def test_same_bits_again_alone_permuted_and_widened(tap, name):
    S, D, K = SYSTEMS[name]
    n = S.shape[0]
    tol = 1e-10
    L = np.tril(S)
    B = pp.columns(name, S, 63)
    X, rc, st = tap.pcg_panel_solve(L, B, D, tol, max_iterations=n)
    it = tap.pcg_panel_columns(63)["iterations"]
    assert rc == 0
    tap.pcg_panel_solve(np.tril(SYSTEMS["partial_single_tile"][0]), np.ones((43, 2)), 6, 1e-6)   # another shape in between
    X2, rc2, _ = tap.pcg_panel_solve(L, B, D, tol, max_iterations=n)
    assert rc2 == 0 and np.array_equal(X, X2)
    for j in (0, 1, 4, 62):
        x1, rc1, _ = tap.pcg_panel_solve(L, B[:, [j]], D, tol, max_iterations=n)
        assert rc1 == 0 and np.array_equal(x1[:, 0], X[:, j]), j
        assert tap.pcg_panel_columns(1)["iterations"][0] == it[j]
    perm = np.random.default_rng(1).permutation(63)
    Xp, rcp, _ = tap.pcg_panel_solve(L, B[:, perm], D, tol, max_iterations=n)
    assert rcp == 0 and np.array_equal(Xp, X[:, perm])
    assert np.array_equal(tap.pcg_panel_columns(63)["iterations"], it[perm])
    B65 = np.c_[pp.columns(name, S, 65, seed=1)[:, :2], B]   # m = 65: the columns move by two, column 62 into the second block
    Xw, rcw, _ = tap.pcg_panel_solve(L, B65, D, tol, max_iterations=n)
    assert rcw == 0 and np.array_equal(Xw[:, 2:], X)
    x64, _, _ = tap.pcg_panel_solve(L, B65[:, [64]], D, tol, max_iterations=n)   # m = 65 against m = 1
    assert np.array_equal(x64[:, 0], Xw[:, 64])


def test_breakdown_beside_healthy_columns(tap):
    S, D, B = pp.breakdown_system()
    n = S.shape[0]
    X, rc, st = tap.pcg_panel_solve(np.tril(S), B, D, 1e-10, max_iterations=n)
    col = tap.pcg_panel_columns(6)
    assert rc == 4 and st["broken_down"] == 1 and st["converged"] == 5 and st["capped"] == 0, st
    assert list(col["breakdown"]) == [1, 0, 0, 0, 0, 0] and list(col["converged"]) == [0, 1, 1, 1, 1, 1]
    assert np.all(np.isfinite(X))
    pp.assert_panel_bounds(S[60:, 60:], np.linalg.cond(S[60:, 60:]), B[60:, 1:], X[60:, 1:], 1e-10, range(5))
    assert np.all(X[:60, 1:] == 0.0)
    X2, rc2, _ = tap.pcg_panel_solve(np.tril(S), B[:, 1:], D, 1e-10, max_iterations=n)
    assert rc2 == 0 and np.array_equal(X2, X[:, 1:])
    # a cap is not an error, and it is reported per column
    Sc = SYSTEMS["composite"][0]
    Xc, rcc, stc = tap.pcg_panel_solve(np.tril(Sc), pp.columns("composite", Sc, 6), 6, 1e-10, max_iterations=5)
    colc = tap.pcg_panel_columns(6)
    assert rcc == 0 and stc["capped"] == 3 and stc["converged"] == 3
    assert list(colc["converged"]) == [1, 0, 1, 0, 0, 1] and list(colc["iterations"]) == [1, 5, 0, 5, 5, 1]


def test_tap_refusals(tap):
    S = SYSTEMS["partial_single_tile"][0]
    n = S.shape[0]
    B = np.ones((n, 2))
    with pytest.raises(hipapi.HipError, match="coarse_aggregate must be 0"):
        tap.pcg_panel_solve(np.tril(S), B, 6, 1e-8, coarse_aggregate=2)
    with pytest.raises(hipapi.HipError, match="m == 0"):
        tap.pcg_panel_solve(np.tril(S), np.zeros((n, 0)), 6, 1e-8)
    with pytest.raises(hipapi.HipError, match="513 columns requested"):
        tap.pcg_panel_solve(np.tril(S), np.zeros((n, 513)), 6, 1e-8)
    with pytest.raises(hipapi.HipError, match="rel_tolerance"):
        tap.pcg_panel_solve(np.tril(S), B, 6, 1.5)
    X, rc, _ = tap.pcg_panel_solve(np.tril(S), B, 6, 1e-10)
    assert rc == 0
    pp.assert_panel_bounds(S, np.linalg.cond(S), B, X, 1e-10, range(2))


# ---- scenes ------------------------------------------------------------------------------------------------------
TOL = 1e-10


def _scene():
    sc = scene.make_scene(44, 300, 6, lm_dim=1, seed=12)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    return sc, pa


def _pcg_solved(sc, pa, **kw):
    s = _engine(sc, 1, pa, **kw)
    s.eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=TOL)
    s.eng.linearize()
    assert s.eng.solve_gn() == 0 and s.eng.pcg_stats()["converged"] == 1
    return s


def _block_err(G, want):
    return np.linalg.norm(G - want, 2) / np.linalg.norm(want, 2)


def _scene_checks(s, direct, pairs, calibration=False):
    eng = s.eng
    S = _sym(eng.get_S())
    n = S.shape[0]
    assert n == eng.num_pose_params() + eng.num_calib_params()
    cond = np.linalg.cond(S)
    assert cond < 1e8, "the scene is too ill-conditioned for the check: %g" % cond
    bound = cond * TOL + 4.5 * EPS * cond
    b = eng.get_rhs()[0]
    # the right-hand side of the step: one column, against the direct solver's step and numpy
    x1, rc = eng.pcg_panel_solve_system(b, TOL)
    assert rc == 0 and x1.shape == (n,)
    d_direct = direct.eng.get_delta_gn()[0]
    e_direct = np.linalg.norm(x1 - d_direct) / np.linalg.norm(d_direct)
    pp.assert_panel_bounds(S, cond, b[:, None], x1[:, None], TOL, [0])
    # 65 random columns
    B = np.random.default_rng(5).standard_normal((n, 65))
    X, rc = eng.pcg_panel_solve_system(B, TOL)
    st = eng.pcg_panel_stats()
    col = eng.pcg_panel_columns(65)
    assert rc == 0 and st["columns"] == 65 and st["column_blocks"] == 2 and st["converged"] == 65, st
    assert np.all(col["converged"] == 1) and col["rel_residual_true"].max() == st["max_rel_residual_true"] <= TOL
    worst = pp.assert_panel_bounds(S, cond, B, X, TOL, range(65))
    assert st["solve_ms"] > 0 and st["spmm_ms"] > 0 and st["workspace_bytes"] > 0 and st["bytes_read_per_product"] > 0
    X2, _ = eng.pcg_panel_solve_system(B, TOL)
    assert np.array_equal(X, X2)
    # joint covariances without a factor
    rows = _natural_rows(s.pa)
    Si = np.linalg.inv(S)
    errs = []
    for ids in pairs:
        r = [rows[p] + x for p in ids for x in range(6)] + (list(range(n - s.K, n)) if calibration else [])
        G = eng.joint_marginals_pcg(ids, include_calibration=calibration, rel_tolerance=TOL)
        assert G.shape == (len(r), len(r)) and np.array_equal(G, G.T)
        e_inv = _block_err(G, Si[np.ix_(r, r)])
        e_dir = _block_err(G, direct.eng.joint_marginals(ids, include_calibration=calibration))
        errs.append((e_inv, e_dir))
        assert e_inv <= bound and e_dir <= bound, (ids, e_inv, e_dir, bound)
    print("n = %d, cond %.2e: step against the direct solver %.2e, 65 columns residual %.2e forward %.2e, joint blocks %s "
          "(bound %.2e); %s" % (n, cond, e_direct, worst[0], worst[1], errs, bound, st))
    assert e_direct <= bound
    return X


def _direct_twin(sc, pa, **kw):
    d = _engine(sc, 1, pa, **kw)
    d.eng.linearize()
    assert d.eng.solve_gn() == 0
    return d


def test_scene_under_every_pose_ordering(monkeypatch):
    sc, pa = _scene()
    act = [int(p) for p in np.nonzero(pa)[0]]
    nact = len(act)
    perm = ((np.arange(nact) + 5) % nact).astype(np.uint32)   # a rotation by 30 rows: not tile aligned
    direct = _direct_twin(sc, pa)
    res = {}
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO, hipapi.ORDER_USER):
        with monkeypatch.context() as mp:
            if mode == hipapi.ORDER_USER:   # _engine sets the mode; the permutation goes with it
                plain = hipapi.Engine.set_pose_ordering
                mp.setattr(hipapi.Engine, "set_pose_ordering",
                           lambda self, md: (plain(self, md), self.set_pose_permutation(perm))[0])
            s = _pcg_solved(sc, pa, mode=mode)
        if mode == hipapi.ORDER_USER:
            assert np.array_equal(s.eng.get_pose_ordering()[0], perm)
        res[mode] = _scene_checks(s, direct, [[act[3], act[4]], [act[1], act[-1]]])
        S = _sym(s.eng.get_S())
        s.eng.close()
    cond = np.linalg.cond(S)
    for mode in (hipapi.ORDER_AUTO, hipapi.ORDER_USER):   # the caller's rows under every ordering
        d = np.linalg.norm(res[mode] - res[hipapi.ORDER_NATURAL], axis=0) / np.linalg.norm(res[hipapi.ORDER_NATURAL], axis=0)
        assert d.max() <= 2 * (cond * TOL + 4.5 * EPS * cond)
    direct.eng.close()


def test_scene_with_calibration_rows():
    """DoTvs: the six calibration rows come last, are one preconditioner block and straddle a tile.  With pose-pose
    terms, as in test_factor_solve_gpu: projection residuals alone leave S singular to working precision once T_vs is
    a parameter (cond 1e18), and random columns then break down in the single-column solver as well."""
    sc, pa = _scene()
    direct = _direct_twin(sc, pa, tvs=True, pose_pose=True)
    s = _pcg_solved(sc, pa, tvs=True, pose_pose=True)
    n = s.eng.num_pose_params() + s.eng.num_calib_params()
    assert s.eng.num_calib_params() == 6 and (n - 6) // 64 != (n - 1) // 64
    act = [int(p) for p in np.nonzero(pa)[0]]
    _scene_checks(s, direct, [[act[2], act[3]], [act[0], act[-1]]], calibration=True)
    s.eng.close()
    direct.eng.close()


def test_refusals_each_with_its_message():
    from ba_amd import sharding
    sc, pa = _scene()
    d = _direct_twin(sc, pa)
    n = d.eng.num_pose_params()
    B = np.ones((n, 3))
    act = [int(p) for p in np.nonzero(pa)[0]]
    for call in (lambda e: e.pcg_panel_solve_system(B), lambda e: e.joint_marginals_pcg(act[:2])):
        with pytest.raises(hipapi.HipError, match="ran the direct solver"):
            call(d.eng)
    d.eng.close()
    s = _engine(sc, 1, pa)
    with pytest.raises(hipapi.HipError, match="needs a PCG solve by the last ba_hip_solve_gn"):
        s.eng.pcg_panel_solve_system(B)
    s.eng.close()
    s = _pcg_solved(sc, pa)
    eng = s.eng
    good, rc = eng.pcg_panel_solve_system(B, TOL)
    assert rc == 0
    with pytest.raises(hipapi.HipError, match="m == 0"):
        eng.pcg_panel_solve_system(np.zeros((n, 0)))
    with pytest.raises(hipapi.HipError, match="513 columns requested, the limit is BA_HIP_PCG_PANEL_MAX_COLUMNS \\(512\\)"):
        eng.pcg_panel_solve_system(np.zeros((n, 513)))
    o = hipapi.PcgOptions(1e-8, 0, 0, 0)
    import ctypes as C
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_pcg_panel_solve_system(eng.h, 3, None, None, C.byref(o)))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_pcg_panel_solve_system(eng.h, 3, B.ctypes.data_as(hipapi.dp), good.ctypes.data_as(hipapi.dp), None))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_pcg_panel_stats(eng.h, None))
    with pytest.raises(hipapi.HipError, match="coarse_aggregate must be 0"):
        eng.pcg_panel_solve_system(B, coarse_aggregate=2)
    with pytest.raises(hipapi.HipError, match="coarse_aggregate must be 0"):
        eng.joint_marginals_pcg(act[:2], coarse_aggregate=2)
    with pytest.raises(hipapi.HipError, match="is repeated"):
        eng.joint_marginals_pcg([act[0], act[0]])
    with pytest.raises(hipapi.HipError, match="not an active pose"):
        eng.joint_marginals_pcg([int(sc.anchor_poses[0])])
    with pytest.raises(hipapi.HipError, match="the limit is BA_HIP_PCG_PANEL_MAX_COLUMNS"):
        eng.joint_marginals_pcg((act * 3)[:90])   # 540 columns
    with pytest.raises(hipapi.HipError, match="m differs"):
        eng.pcg_panel_columns(7)
    # the existing getter keeps refusing under PCG
    with pytest.raises(hipapi.HipError, match="PCG"):
        eng.joint_marginals(act[:2])
    again, _ = eng.pcg_panel_solve_system(B, TOL)
    assert np.array_equal(again, good)
    full, rc = eng.pcg_panel_solve_system(np.ones((n, 512)), 1e-6)   # the limit itself: eight column blocks
    assert rc == 0 and np.array_equal(full[:, 0], full[:, 511]) and np.all(np.isfinite(full))
    eng.linearize()
    for call in (lambda: eng.pcg_panel_solve_system(B), lambda: eng.joint_marginals_pcg(act[:2])):
        with pytest.raises(hipapi.HipError, match="re-linearised since the PCG solve"):
            call()
    assert eng.solve_gn() == 0
    assert eng.pcg_panel_solve_system(B, TOL)[1] == 0
    eng.close()
    ar = sharding.ThreadAllReduce(2)
    eng = hipapi.Engine(1, 6)
    eng.set_allreduce(ar.hook(0), 0, 2)
    with pytest.raises(hipapi.HipError, match="ba_hip_pcg_panel_solve_system: not available on a sharded engine"):
        eng.pcg_panel_solve_system(np.ones(0))
    with pytest.raises(hipapi.HipError, match="ba_hip_get_joint_marginals_pcg: not available on a sharded engine"):
        eng.joint_marginals_pcg([1, 2])
    eng.close()


def test_new_calls_leave_the_engine_alone_and_return_their_memory():
    sc, pa = _scene()
    act = [int(p) for p in np.nonzero(pa)[0]]
    live = hipapi.device_bytes_live()
    s, twin = _pcg_solved(sc, pa), _pcg_solved(sc, pa)
    eng = s.eng
    n = eng.num_pose_params()
    before = (eng.get_delta_gn(), eng.pcg_stats(), eng.get_S())
    held = hipapi.device_bytes_live()
    B = np.random.default_rng(2).standard_normal((n, 70))
    assert eng.pcg_panel_solve_system(B, 1e-8)[1] == 0
    eng.joint_marginals_pcg(act[:3], rel_tolerance=1e-8)
    with pytest.raises(hipapi.HipError):
        eng.pcg_panel_solve_system(B, coarse_aggregate=2)
    assert hipapi.device_bytes_live() - held == eng.pcg_panel_stats()["workspace_bytes"] > 0
    after = (eng.get_delta_gn(), eng.pcg_stats(), eng.get_S())
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert before[1] == after[1] and np.array_equal(before[2], after[2])
    res, rhs = eng.check_solve()   # pcg_solved is still set: the tap runs on S in A
    assert res <= (TOL + 1e-9) * rhs
    for e in (eng, twin.eng):      # the next Gauss-Newton iteration
        e.compose_step(0.0, 1.0)
        e.apply_step()
        e.linearize()
        assert e.solve_gn() == 0
    for a, b in zip(eng.get_delta_gn(), twin.eng.get_delta_gn()):
        assert np.array_equal(a, b)
    assert eng.pcg_stats()["iterations"] == twin.eng.pcg_stats()["iterations"]
    assert np.array_equal(eng.get_S(), twin.eng.get_S())
    eng.close()
    twin.eng.close()
    assert hipapi.device_bytes_live() == live


# ---- through the class and the demo --------------------------------------------------------------------------
def test_class_solve_with_pcg_and_iterative_joint_covariance():
    from ba_amd import adjuster
    from helpers import fill
    from test_pcg_gpu import direct_options, pcg_options
    sc = scene.make_scene(60, 240, 6, lm_dim=1, seed=21)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    act = [int(p) for p in np.nonzero(pa)[0]]
    p, d = adjuster.BundleAdjuster(1, 6), adjuster.BundleAdjuster(1, 6)
    p.Init(pcg_options(pcg_tolerance=TOL))
    d.Init(direct_options())
    for h in (p, d):
        fill(h, sc, active=pa)
        h.Solve(1)
    S = _sym(p.engine().get_S())   # of the linearisation the solve ran on: the applied step does not touch A
    n = S.shape[0]
    cond = np.linalg.cond(S)
    bound = cond * TOL + 4.5 * EPS * cond
    B = np.random.default_rng(3).standard_normal((n, 7))
    X = p.SolveWithPcg(B, TOL)
    pp.assert_panel_bounds(S, cond, B, X, TOL, range(7))
    assert np.array_equal(p.SolveWithPcg(B), X)   # tol 0: Options::pcg_tolerance, the same 1e-10
    st = p.GetPcgPanelStats()
    assert st["columns"] == 7 and st["converged"] == 7 and st["passes"] > 0
    ids = [act[0], act[-1], act[7]]
    G = p.GetJointPoseCovarianceIterative(ids, TOL)
    want = d.GetJointPoseCovariance(ids)
    assert G.shape == (18, 18) and _block_err(G, want) <= bound
    with pytest.raises(RuntimeError, match="unavailable"):
        d.SolveWithPcg(B)
    with pytest.raises(RuntimeError, match="unavailable"):
        d.GetJointPoseCovarianceIterative(ids)
    with pytest.raises(RuntimeError, match="unavailable"):   # the factor getter keeps refusing under PCG
        p.GetJointPoseCovariance(ids)


def test_demo_application_prints_a_joint_block():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ba_amd", "lib", "visual_ba_demo")
    r = subprocess.run([exe, "--pcg", "1e-10", "--joint-cov", "2,23"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "joint covariance of poses 2 and 23 by the panel PCG: 12 columns" in r.stdout and "12 converged" in r.stdout
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(" ") and len(ln.split()) == 12]
    G = np.array(rows[-12:], dtype=np.float64)
    assert G.shape == (12, 12) and np.array_equal(G, G.T) and np.all(np.diag(G) > 0)
    r = subprocess.run([exe, "--joint-cov", "2,23"], capture_output=True, text=True, timeout=120)   # without --pcg: refused
    assert r.returncode == 2 and "iterative joint covariance unavailable" in r.stdout
