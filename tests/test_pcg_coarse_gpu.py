"""The two-level preconditioner of the PCG solve on the MI355X (ba_hip_pcg_options.coarse_aggregate,
k_pcg_coarse.hip): the stand-alone solver on the families of tests/pcg_cases.py with the bounds and the iteration
counts of the host restatement, the coarse matrix and its explicit inverse through the tap, coarse dimensions at the
tile edge, the cap and the breakdowns; through the engine on the oracle's 200-pose scene, under a reversed pose
permutation (equal bits of C), with calibration unknowns and masked parameters; option 0 against today's callers;
and through the class."""
import numpy as np
import pytest

import pcg_cases as pc
import pcg_coarse_cases as cc
from ba_amd import adjuster, hipapi, scene
from helpers import fill, rel_err

pytestmark = pytest.mark.gpu

FAMILIES = pc.families()


@pytest.fixture(scope="module")
def hc():
    return cc.host_lib()


def check_coarse_tap(eng, S, Z):
    """C within the summation bound, C C^-1 = I within 8 nc eps cond2(C), C^-1 symmetric to the bit"""
    C, Cinv = eng.pcg_coarse()
    ref, bound = cc.coarse_reference(S, Z)
    assert C.shape == ref.shape
    assert np.all(np.abs(C - ref) <= bound), np.max(np.abs(C - ref) / np.maximum(bound, 1e-300))
    assert np.array_equal(C, C.T)
    nc = C.shape[0]
    defect = np.max(np.abs(C @ Cinv - np.eye(nc)))
    cap = 8 * nc * cc.EPS * np.linalg.cond(C)
    print("coarse space %d: max |C C^-1 - I| %.2e (bound %.2e)" % (nc, defect, cap))
    assert defect <= cap
    assert np.array_equal(Cinv, Cinv.T)
    return C, Cinv


# ---- stand-alone solver ------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_two_level_pcg_solve_matrix_families(hc, name, tol):
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    g = cc.FAMILY_G[name]
    b = pc.rhs_for(S)
    # ba_hip_pcg_solve takes one block size: the border rows fall into blocks (and aggregates) like the rest
    Z, g_used, naggr = cc.aggregation(n, D, 0, g)
    eng = hipapi.Engine(1, 6)
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, tol, max_iterations=n, coarse_aggregate=g)
    assert rc == 0 and st["converged"] == 1 and st["breakdown"] == 0, st
    cst = eng.pcg_coarse_stats()
    assert (cst["aggregate_used"], cst["coarse_unknowns"], cst["aggregates"]) == (g_used, Z.shape[1], naggr), cst
    rel = pc.assert_residual(S, b, x, tol)
    err = pc.assert_forward_error(S, b, x, tol)
    check_coarse_tap(eng, S, Z)
    xh, rch, sth = cc.host_pcg2(hc, S, b, D, 0, tol, g, max_it=n)
    assert rch == 0 and st["iterations"] == sth["iterations"], (st["iterations"], sth["iterations"])
    x2, rc2, st2 = eng.pcg_solve(np.tril(S), b, D, tol, max_iterations=n, coarse_aggregate=g)
    assert rc2 == 0 and np.array_equal(x, x2)
    assert st2["iterations"] == st["iterations"] and st2["rel_residual_true"] == st["rel_residual_true"]
    print("%s tol %.0e g %d: %d iterations, residual %.2e, forward error %.2e, solve %.3f ms (setup %.3f ms, %.1f us per pass)"
          % (name, tol, g, st["iterations"], rel, err, st["solve_ms"], cst["setup_ms"], 1e3 * cst["apply_ms"]))
    eng.close()


def _banded_spd(n, seed):
    rng = np.random.default_rng(seed)
    S = np.diag(2.0 + rng.random(n))
    S += np.diag(0.5 * np.ones(n - 1), 1) + np.diag(0.5 * np.ones(n - 1), -1)
    return S


@pytest.mark.parametrize("n", [64, 65])
def test_coarse_dimension_at_the_tile_edge(hc, n):
    """block 1, g = 1: the coarse matrix is S itself, exactly one tile / one tile and one row"""
    S = _banded_spd(n, n)
    b = pc.rhs_for(S, 6)
    Z, _, _ = cc.aggregation(n, 1, 0, 1)
    eng = hipapi.Engine(1, 6)
    x, rc, st = eng.pcg_solve(np.tril(S), b, 1, 1e-10, coarse_aggregate=1)
    assert rc == 0 and st["converged"] == 1, st
    assert eng.pcg_coarse_stats()["coarse_unknowns"] == n
    pc.assert_residual(S, b, x, 1e-10)
    C, Cinv = check_coarse_tap(eng, S, Z)
    assert np.array_equal(C, S)
    assert st["iterations"] == cc.host_pcg2(hc, S, b, 1, 0, 1e-10, 1)[2]["iterations"]
    eng.close()


def test_aggregate_grows_until_the_coarse_space_fits(hc):
    n = 1100
    S = _banded_spd(n, 7)
    b = pc.rhs_for(S, 5)
    Z, g_used, _ = cc.aggregation(n, 1, 0, 1)
    assert g_used == 2
    eng = hipapi.Engine(1, 6)
    x, rc, st = eng.pcg_solve(np.tril(S), b, 1, 1e-8, coarse_aggregate=1)
    assert rc == 0 and st["converged"] == 1, st
    cst = eng.pcg_coarse_stats()
    assert cst["aggregate_used"] == 2 and cst["coarse_unknowns"] == 550 and cst["aggregates"] == 550, cst
    pc.assert_residual(S, b, x, 1e-8)
    check_coarse_tap(eng, S, Z)
    assert st["iterations"] == cc.host_pcg2(hc, S, b, 1, 0, 1e-8, 1)[2]["iterations"]
    eng.close()


def test_one_iteration_and_the_breakdowns():
    eng = hipapi.Engine(1, 6)
    S = pc.block_diagonal()
    b = pc.rhs_for(S, 1)
    x, rc, st = eng.pcg_solve(np.tril(S), b, 6, 1e-10, coarse_aggregate=1)   # M^-1 = 2 S^-1
    assert rc == 0 and st["converged"] == 1 and st["iterations"] == 1, st
    pc.assert_residual(S, b, x, 1e-10)
    # the blocks are fine, the coarse matrix (S itself) is indefinite
    S, D, b = pc.indefinite_with_spd_blocks()
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, 1e-12, max_iterations=S.shape[0], coarse_aggregate=1)
    assert rc == 4 and st["breakdown"] == 4 and st["converged"] == 0 and np.all(x == 0.0), st
    # a block that is not positive definite is named first
    S, D = pc.negative_block()
    x, rc, st = eng.pcg_solve(np.tril(S), pc.rhs_for(S, 2), D, 1e-8, coarse_aggregate=1)
    assert rc == 4 and st["breakdown"] == 3 and st["converged"] == 0 and np.all(x == 0.0), st
    # the engine is still usable, and a solve without the coarse space has no coarse statistics
    S, D, K = FAMILIES["banded_D6"]
    b = pc.rhs_for(S)
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, 1e-10)
    assert rc == 0 and st["converged"] == 1
    with pytest.raises(hipapi.HipError, match="did not use the coarse space"):
        eng.pcg_coarse_stats()
    eng.close()


# ---- through the engine ----------------------------------------------------------------------------------
def _engine(sc, pa, perm=None, calib=False, masks=None):
    eng = hipapi.Engine(1, 6)
    if calib:
        eng.set_calibration(0, True)
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::sc.obs_per_landmark + 1] = False
    eng.set_cameras(sc.cam_params, [0.01, -0.02, 0.03, 0, 0, 0, 1] if calib else [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    if perm is not None:
        eng.set_pose_ordering(hipapi.ORDER_USER)
        eng.set_pose_permutation(perm)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16) if masks is None else masks)
    return eng


def _sym(eng):
    U = np.triu(eng.get_S())
    return U + np.triu(U, 1).T


def test_engine_200_pose_scene_against_the_oracle_and_the_host_restatement(hc, oracle_lib):
    from helpers import gn_options
    po = oracle_lib
    sc = scene.make_scene(200, 20000, 10, lm_dim=1, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o = po.OracleBundleAdjuster(1, 6)
    o.Init(gn_options(po, apply_results=0))
    fill(o, sc, active=pa)
    o.Solve(1)
    for tol in (1e-6, 1e-8):
        h = adjuster.BundleAdjuster(1, 6)
        h.Init(_options(reduced_solver=1, pcg_tolerance=tol, pcg_max_iterations=1188, pcg_coarse_aggregate=10, apply_results=0))
        fill(h, sc, active=pa)
        h.Solve(1)
        eng = h.engine()
        n = eng.num_pose_params()
        assert n == 1188
        st, cst = eng.pcg_stats(), eng.pcg_coarse_stats()
        assert st["converged"] == 1, st
        assert (cst["aggregate_used"], cst["coarse_unknowns"], cst["aggregates"]) == (10, 120, 20), cst
        S = _sym(eng)            # S is intact after a PCG solve
        b = eng.get_rhs()[0]
        x = eng.get_delta_gn()[0]
        rel = pc.assert_residual(S, b, x, tol)
        # the oracle's step solves its own S, equal to this one to 1e-12 (test_gpu_parity): cond (tol + 4.5 eps + 1e-12)
        cond = np.linalg.cond(S)
        err = rel_err(x, o.delta_p())
        assert err <= cond * (tol + 4.5 * pc.EPS + 1e-12), (err, cond)
        Z, _, _ = cc.aggregation(n, 6, 0, 10)
        check_coarse_tap(eng, S, Z)
        xh, rch, sth = cc.host_pcg2(hc, S, b, 6, 0, tol, 10, max_it=n)
        assert rch == 0 and st["iterations"] == sth["iterations"], (st["iterations"], sth["iterations"])
        print("200 poses, tol %.0e, g = 10: %d iterations, residual %.2e, step vs oracle %.2e, solve %.3f ms (setup %.3f ms, "
              "%.1f us per pass, %.1f us per product)" % (tol, st["iterations"], rel, err, st["solve_ms"], cst["setup_ms"],
                                                          1e3 * cst["apply_ms"], 1e3 * st["spmv_ms"]))


def test_engine_reversed_pose_permutation_gives_the_bits_of_natural_order():
    """Aggregates are defined in pose-id order and every entry of C is one sum over its fine rows in that order:
    where ORDER_USER puts the rows does not change a bit of C — given the same bits of S
    (test_pcg_coarse_plan.test_coarse_matrix_does_not_depend_on_where_a_pose_ordering_puts_the_rows), which the
    Schur complement provides: the V^-1-weighted factor of every pair term is that of the pose with the smaller pose
    id, under any ordering.  Measured: S and C equal in every bit, 32 / 32 iterations.  DESIGN section 13a."""
    sc = scene.make_scene(60, 600, 6, lm_dim=1, seed=21)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    nact = int(pa.sum())
    out = []
    for perm in (None, np.arange(nact, dtype=np.uint32)[::-1].copy()):
        eng = _engine(sc, pa, perm=perm)
        n = eng.num_pose_params()
        eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-10, max_iterations=n, coarse_aggregate=4)
        eng.linearize()
        assert eng.solve_gn() == 0
        st = eng.pcg_stats()
        assert st["converged"] == 1, st
        S = _sym(eng)            # taps are in natural order under any ordering
        pc.assert_residual(S, eng.get_rhs()[0], eng.get_delta_gn()[0], 1e-10)
        out.append((eng.pcg_coarse(), S, eng.get_delta_gn()[0], st["iterations"]))
        eng.close()
    (C0, _), S0, x0, it0 = out[0]
    (C1, _), S1, x1, it1 = out[1]
    assert C0.shape == (6 * -(-nact // 4),) * 2
    dS, dC = S0 != S1, C0 != C1
    print("reversed permutation: iterations %d / %d, steps differ by %.2e; S differs in %d of %d entries (max rel. %.2e, "
          "%d of them on the 6 x 6 diagonal blocks), C in %d of %d (max rel. %.2e)"
          % (it0, it1, rel_err(x1, x0), dS.sum(), dS.size, np.max(np.abs(S0 - S1) / np.maximum(np.abs(S0), 1e-300)),
             sum(dS[6 * a:6 * a + 6, 6 * a:6 * a + 6].sum() for a in range(nact)), dC.sum(), dC.size,
             np.max(np.abs(C0 - C1) / np.maximum(np.abs(C0), 1e-300))))
    assert np.array_equal(S0, S1)      # the Schur complement itself does not depend on the ordering (structure.h)
    assert np.array_equal(C0, C1)


@pytest.mark.parametrize("kind", ["calibration", "masked"])
def test_engine_calibration_unknowns_and_masked_parameters(hc, kind):
    sc = scene.make_scene(30, 60, 5, lm_dim=1, seed=7)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    masks = None
    if kind == "masked":
        masks = np.zeros(sc.num_poses, dtype=np.uint16)
        masks[np.flatnonzero(pa)[:3]] = 0b000111      # three poses with their first three parameters held
    else:
        pa[::3] = 0
    eng = _engine(sc, pa, calib=kind == "calibration", masks=masks)
    n, K = eng.num_pose_params(), eng.num_calib_params()
    assert (K > 0) == (kind == "calibration")
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-10, max_iterations=n + K, coarse_aggregate=4)
    eng.linearize()
    assert eng.solve_gn() == 0
    st, cst = eng.pcg_stats(), eng.pcg_coarse_stats()
    assert st["converged"] == 1, st
    nact = n // 6
    assert cst["coarse_unknowns"] == 6 * -(-nact // 4) + K and cst["aggregates"] == -(-nact // 4), cst
    S = _sym(eng)
    b = eng.get_rhs()[0]
    pc.assert_residual(S, b, eng.get_delta_gn()[0], 1e-10)
    Z, _, _ = cc.aggregation(n + K, 6, K, 4)
    check_coarse_tap(eng, S, Z)
    sth = cc.host_pcg2(hc, S, b, 6, K, 1e-10, 4, max_it=n + K)[2]
    assert st["iterations"] == sth["iterations"], (st["iterations"], sth["iterations"])
    eng.close()


def test_option_0_gives_the_bits_of_todays_callers_and_switches_without_finalize():
    sc = scene.make_scene(60, 600, 6, lm_dim=1, seed=21)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    eng, ref = _engine(sc, pa), _engine(sc, pa)
    n = eng.num_pose_params()
    # `ref` fills the struct as callers written before the option do: three zeroed reserved words
    o = hipapi.PcgOptions(1e-8, n, 0)
    ref._chk(ref.L.ba_hip_set_reduced_solver(ref.h, hipapi.SOLVER_PCG, hipapi.C.byref(o)))
    ref.linearize()
    assert ref.solve_gn() == 0
    x_ref, it_ref = ref.get_delta_gn()[0], ref.pcg_stats()["iterations"]
    with pytest.raises(hipapi.HipError, match="did not use the coarse space"):
        ref.pcg_coarse_stats()
    steps = []
    for g in (0, 5, 0):      # no finalize between the three
        eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8, max_iterations=n, coarse_aggregate=g)
        eng.linearize()
        assert eng.solve_gn() == 0
        st = eng.pcg_stats()
        assert st["converged"] == 1, st
        steps.append((eng.get_delta_gn()[0], st["iterations"]))
        if g:
            assert eng.pcg_coarse_stats()["aggregate_used"] == 5
        else:
            with pytest.raises(hipapi.HipError, match="did not use the coarse space"):
                eng.pcg_coarse_stats()
    assert np.array_equal(steps[0][0], x_ref) and steps[0][1] == it_ref
    assert np.array_equal(steps[2][0], x_ref) and steps[2][1] == it_ref
    # both steps solve the same S to 1e-8 relative residual: they differ by at most 2 cond2(S) 1e-8
    assert steps[1][1] < it_ref and rel_err(steps[1][0], x_ref) <= 2 * np.linalg.cond(_sym(eng)) * 1e-8
    print("option 0 / 5 / 0: %d / %d / %d iterations" % (steps[0][1], steps[1][1], steps[2][1]))
    eng.close()
    ref.close()


def test_coarse_tables_follow_the_system_when_the_work_space_changes_hands():
    """g = 5 on the engine's scene, then the stand-alone solver with g = 5 on another system (the device tables now
    describe that one), then the engine with the option off (every other table is uploaded again), then g = 5 once
    more: the last solve must give the bits of the first, C included — not run with the other system's aggregates."""
    sc = scene.make_scene(60, 600, 6, lm_dim=1, seed=21)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    eng = _engine(sc, pa)
    n = eng.num_pose_params()

    def solve(g):
        eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8, max_iterations=n, coarse_aggregate=g)
        eng.linearize()
        assert eng.solve_gn() == 0
        st = eng.pcg_stats()
        assert st["converged"] == 1, st
        return eng.get_delta_gn()[0], st["iterations"]

    x_first, it_first = solve(5)
    C_first = eng.pcg_coarse()[0]
    S, D, K = FAMILIES["banded_D15"]            # 300 rows in blocks of 15: other rows, other aggregates, same g
    xs, rc, st = eng.pcg_solve(np.tril(S), pc.rhs_for(S), D, 1e-8, coarse_aggregate=5)
    assert rc == 0 and st["converged"] == 1, st
    x_off, it_off = solve(0)
    x_again, it_again = solve(5)
    assert it_again == it_first and np.array_equal(x_again, x_first)
    assert np.array_equal(eng.pcg_coarse()[0], C_first)
    assert it_off > it_first
    eng.close()


# ---- through the class -----------------------------------------------------------------------------------
def _options(**kw):
    o = adjuster.default_options()
    o.use_dogleg = 0
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_class_five_iterations_track_the_direct_solver():
    """Options::pcg_coarse_aggregate through ba::BundleAdjuster and ba_adjuster_*: five Gauss-Newton iterations at
    tolerance 1e-6 end at the direct solver's projection error to 1e-6 relative (DESIGN section 13's criterion)."""
    sc = scene.make_scene(60, 600, 6, lm_dim=1, seed=21)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    runs = []
    for opts in (_options(reduced_solver=1, pcg_tolerance=1e-6, pcg_coarse_aggregate=4), _options(reduced_solver=0)):
        h = adjuster.BundleAdjuster(1, 6)
        h.Init(opts)
        fill(h, sc, active=pa)
        for it in range(5):
            h.Solve(1)
            if opts.reduced_solver:
                st, cst = h.GetPcgStats(), h.GetPcgCoarseStats()
                assert st is not None and st["converged"] == 1, (it, st)
                assert cst is not None and cst["aggregate_used"] == 4 and cst["coarse_unknowns"] == 6 * -(-int(pa.sum()) // 4), cst
            else:
                assert h.GetPcgCoarseStats() is None
        runs.append(h.summary().proj_error)
    print("five iterations: proj_error %.10e (two-level PCG) / %.10e (direct)" % tuple(runs))
    assert abs(runs[0] - runs[1]) <= 1e-6 * runs[1]


def test_class_visual_inertial_window_returns():
    """PoseSize 15, dogleg, 30 poses (cond(S) up to 1e14): every Solve(1) returns with a result that
    is not SolverError; whether CG converges there is reported, not asserted."""
    o = adjuster.default_options()
    o.reduced_solver = 1
    o.pcg_tolerance = 1e-8
    o.pcg_coarse_aggregate = 4
    sc = scene.make_scene(30, 300, 6, lm_dim=1, seed=3, outlier_frac=0.0)
    scene.add_inertial(sc, period=60.0 * 30 / 100.0, seed=3)
    a = adjuster.BundleAdjuster(1, 15)
    a.Init(o)
    scene.populate(a, sc, imu=True, priors=True, unary_every=10)
    for it in range(4):
        a.Solve(1)
        s, st, cst = a.summary(), a.GetPcgStats(), a.GetPcgCoarseStats()
        assert adjuster.RESULT_NAMES[s.result] != "SolverError", it
        print("VI window step %d: result %s, pcg %s, coarse %s" % (it + 1, adjuster.RESULT_NAMES[s.result], st and {
            k: st[k] for k in ("iterations", "converged", "breakdown", "rel_residual_true", "rel_residual_recurrence")}, cst))


def test_demo_application_with_the_coarse_space():
    import os
    import subprocess
    exe = os.path.join(cc.ROOT, "ba_amd", "lib", "visual_ba_demo")
    r = subprocess.run([exe, "--pcg", "1e-10", "--pcg-coarse", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step 1: pcg iterations" in r.stdout and "converged 1" in r.stdout and "pcg coarse space" in r.stdout
    print(r.stdout)
