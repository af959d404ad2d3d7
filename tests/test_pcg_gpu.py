"""The iterative reduced solve on the MI355X (ba_hip_set_reduced_solver, ba_hip_pcg_solve; k_pcg.hip): the
stand-alone solver on the matrix families of tests/pcg_cases.py, the engine path on the golden fixtures and on
configs[1] at full size, the C++ class with Options::reduced_solver = Pcg against the direct solver, a system too
large to download checked by ba_hip_check_solve, and the refusals."""
import glob
import os

import numpy as np
import pytest

import pcg_cases as pc
from ba_amd import adjuster, hipapi, scene
from helpers import fill, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "config1_*.npz")))
FAMILIES = pc.families()


def lower_tile_count(S):
    n = S.shape[0]
    nt = (n + 63) // 64
    return sum(1 for i in range(nt) for j in range(i + 1)
               if i == j or np.any(S[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] != 0.0))


# ---- stand-alone solver ------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_pcg_solve_matrix_families(name, tol):
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    b = pc.rhs_for(S)
    eng = hipapi.Engine(1, 6)
    # ba_hip_pcg_solve takes one block size: the border of K rows falls into blocks of D like the rest (M stays
    # the block diagonal of S for that partition)
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, tol, max_iterations=n)
    assert rc == 0 and st["converged"] == 1 and st["breakdown"] == 0, st
    assert st["iterations"] <= n
    rel = pc.assert_residual(S, b, x, tol)
    err = pc.assert_forward_error(S, b, x, tol)
    assert st["tiles_read_per_spmv"] == lower_tile_count(S)
    x2, rc2, st2 = eng.pcg_solve(np.tril(S), b, D, tol, max_iterations=n)
    assert rc2 == 0 and np.array_equal(x, x2)
    assert st2["iterations"] == st["iterations"] and st2["rel_residual_true"] == st["rel_residual_true"]
    print("%s tol %.0e: %d iterations, residual %.2e (reported %.2e), forward error %.2e, %.3f ms"
          % (name, tol, st["iterations"], rel, st["rel_residual_true"], err, st["solve_ms"]))
    eng.close()


def test_pcg_solve_block_diagonal_needs_one_iteration():
    S = pc.block_diagonal()
    b = pc.rhs_for(S, 1)
    eng = hipapi.Engine(1, 6)
    x, rc, st = eng.pcg_solve(np.tril(S), b, 6, 1e-10)
    assert rc == 0 and st["converged"] == 1 and st["iterations"] == 1, st
    pc.assert_residual(S, b, x, 1e-10)
    eng.close()


def test_pcg_solve_breakdowns_and_iteration_cap():
    eng = hipapi.Engine(1, 6)
    S, D = pc.negative_block()
    x, rc, st = eng.pcg_solve(np.tril(S), pc.rhs_for(S, 2), D, 1e-8)
    assert rc == 4 and st["breakdown"] == 3 and st["converged"] == 0 and np.all(x == 0.0), st
    S, D, b = pc.indefinite_with_spd_blocks()
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, 1e-12, max_iterations=S.shape[0])
    assert rc == 4 and st["breakdown"] == 1 and st["converged"] == 0 and np.all(np.isfinite(x)), st
    S, D, K = FAMILIES["banded_D6"]
    b = pc.rhs_for(S, 3)
    b[17] = np.nan
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, 1e-8)
    assert rc == 4 and st["breakdown"] == 2 and st["converged"] == 0 and np.all(np.isfinite(x)), st
    S, D, K = FAMILIES["revisit_3_laps"]
    b = pc.rhs_for(S, 4)
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, 1e-10, max_iterations=3)
    assert rc == 0 and st["converged"] == 0 and st["breakdown"] == 0 and st["iterations"] == 3, st
    assert b @ x > 0.0
    # the engine is still usable
    x, rc, st = eng.pcg_solve(np.tril(S), b, D, 1e-10)
    assert rc == 0 and st["converged"] == 1
    eng.close()


# ---- engine path ---------------------------------------------------------------------------------------
def pcg_options(**kw):
    o = adjuster.default_options()
    o.use_dogleg = 0
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    o.reduced_solver = 1
    o.pcg_tolerance = 1e-10
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def direct_options(**kw):
    return pcg_options(reduced_solver=0, **kw)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_fixtures_with_pcg(path):
    """The assertions of test_gpu_parity.test_golden_fixtures with the PCG solver at 1e-10; S is read after the
    solve WITHOUT keep_reduced_system (write_reduced_camera_matrix stays 0): PCG leaves S in place."""
    g = np.load(path)
    h = adjuster.BundleAdjuster(int(g["lm_dim"]), 6)
    h.Init(pcg_options(use_dogleg=int(g["use_dogleg"]), pcg_max_iterations=288))
    h.AddCamera(g["cam_params"])
    h.add_poses(g["poses"], is_active=g["pose_active"])
    h.add_landmarks(g["landmarks"], g["lm_ref_pose"])
    h.add_projection_residuals(g["obs_z"], g["obs_pose"], g["obs_lm"])
    h.Solve(1)
    st = h.GetPcgStats()
    assert st is not None and st["converged"] == 1 and st["iterations"] <= 288, st
    assert rel_err(h.S(), g["S_it0"]) < 1e-12
    assert rel_err(h.rhs(), g["rhs_it0"]) < 1e-11
    print("%s: %d iterations, delta_p %.2e, delta_l %.2e of the fixture" % (
        os.path.basename(path), st["iterations"], rel_err(h.delta_p(), g["delta_p_it0"]), rel_err(h.delta_l(), g["delta_l_it0"])))
    assert rel_err(h.delta_p(), g["delta_p_it0"]) < 1e-8
    assert rel_err(h.delta_l(), g["delta_l_it0"]) < 1e-8
    assert abs(h.summary().proj_error - float(g["proj_error_it0"])) < 1e-9 * float(g["proj_error_it0"])
    for _ in range(int(g["iters"]) - 1):
        h.Solve(1)
        assert h.GetPcgStats()["converged"] == 1
    t, _, _ = h.poses()
    assert rel_err(t, g["poses_final"]) < 1e-8
    assert rel_err(h.landmarks(), g["landmarks_final"]) < 1e-8


def _engine(sc, pa, revisit=False):
    eng = hipapi.Engine(1, 6)
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    if revisit:
        keep &= ~np.r_[True, np.diff(sc.obs_lm) != 0]   # the reference-frame observation of every landmark
    else:
        keep[::sc.obs_per_landmark + 1] = False
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    return eng


def test_config1_full_size_residual_and_switch_back_to_direct():
    """BASELINE.json configs[1] (n = 5 988) at rel_tolerance 1e-8: S, rhs and the step are downloaded and the residual
    bound is evaluated in numpy; the same engine switched back to DIRECT gives the bits of a direct-only engine."""
    sc = scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    eng = _engine(sc, pa)
    n = eng.num_pose_params()
    assert n == 5988
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8, max_iterations=n)
    eng.linearize()
    assert eng.solve_gn() == 0
    st = eng.pcg_stats()
    assert st["converged"] == 1 and st["iterations"] <= n, st
    U = np.triu(eng.get_S())   # no keep_reduced_system: S is intact after a PCG solve (block upper triangle, as the
    S = U + np.triu(U, 1).T    # reference keeps it: symmetrised here)
    b = eng.get_rhs()[0]
    x = eng.get_delta_gn()[0]
    rel = pc.assert_residual(S, b, x, 1e-8)
    res, rhs = eng.check_solve()   # the dense two-pass product of k_reduce.hip: shares no code with the tile product
    assert abs(rhs - st["rhs_norm"]) <= 1e-12 * rhs
    assert res / rhs <= 1e-8 + 1e-9
    print("configs[1]: %d iterations, %.3f ms (%.1f us per product, %.2f TB/s), residual %.2e numpy / %.2e reported / %.2e check_solve"
          % (st["iterations"], st["solve_ms"], 1e3 * st["spmv_ms"], st["bytes_read_per_spmv"] / max(st["spmv_ms"], 1e-9) / 1e9,
             rel, st["rel_residual_true"], res / rhs))
    x_again = None
    eng.linearize()
    assert eng.solve_gn() == 0
    x_again = eng.get_delta_gn()[0]
    assert np.array_equal(x, x_again) and eng.pcg_stats()["iterations"] == st["iterations"]
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.linearize()
    assert eng.solve_gn() == 0
    with pytest.raises(hipapi.HipError, match="did not run the PCG solver"):
        eng.pcg_stats()
    ref = _engine(sc, pa)
    ref.linearize()
    assert ref.solve_gn() == 0
    for a, r in zip(eng.get_delta_gn(), ref.get_delta_gn()):
        assert np.array_equal(a, r)
    print("configs[1]: direct solve %.3f ms; PCG step vs direct %.2e" % (ref.get_timers()["solve"], rel_err(x, ref.get_delta_gn()[0])))
    eng.close()
    ref.close()


# ---- through the class -----------------------------------------------------------------------------------
def _class_pair(kind):
    """(pcg adjuster, direct adjuster) on the same problem"""
    import test_gpu_parity as tp
    out = []
    if kind in ("lm1_gn", "lm3_gn", "lm1_dogleg", "lm3_dogleg"):
        lm_dim, dog = int(kind[2]), int(kind.endswith("dogleg"))
        sc = scene.make_scene(60, 240, 6, lm_dim=lm_dim, seed=21)
        pa = np.ones(sc.num_poses, dtype=np.uint8)
        pa[sc.anchor_poses] = 0
        for opts in (pcg_options(use_dogleg=dog), direct_options(use_dogleg=dog)):
            h = adjuster.BundleAdjuster(lm_dim, 6)
            h.Init(opts)
            fill(h, sc, active=pa)
            out.append(h)
    elif kind == "tvs":
        from oracle import pyoracle as po
        po.build()
        sc, pa, t0 = tp._calib_scene(po=po, outlier_frac=0.0, pixel_sigma=0.3)
        for opts in (pcg_options(), direct_options()):
            h = adjuster.BundleAdjuster(1, 6, do_tvs=True)
            h.Init(opts)
            h.AddCamera(sc.cam_params, t0)
            h.add_poses(sc.poses, is_active=pa)
            h.add_landmarks(sc.landmarks, sc.lm_ref_pose)
            h.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
            out.append(h)
    elif kind == "calib4":
        sc, pa, wrong = tp._intrinsics_scene(outlier_frac=0.0, pixel_sigma=0.3)
        for opts in (pcg_options(), direct_options()):
            h = adjuster.BundleAdjuster(1, 6, calib_size=4)
            h.Init(opts)
            h.AddCamera(wrong)
            h.add_poses(sc.poses, is_active=pa)
            h.add_landmarks(sc.landmarks, sc.lm_ref_pose)
            h.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)
            out.append(h)
    elif kind == "auto_ordering":
        P = 600
        sc = scene.make_revisit_scene(P, 5 * P, laps=3, window=12, revisit_frac=0.5, seed=0)
        pa = np.ones(P, dtype=np.uint8)
        pa[sc.anchor_poses] = 0
        for opts in (pcg_options(pose_ordering=1), direct_options(pose_ordering=1)):
            h = adjuster.BundleAdjuster(1, 6)
            h.Init(opts)
            fill(h, sc, active=pa)
            out.append(h)
    elif kind == "dense_prior":
        sc = scene.make_scene(30, 300, 6, lm_dim=1, seed=3, outlier_frac=0.0)
        src = adjuster.BundleAdjuster(1, 6)
        src.Init(direct_options())
        scene.populate(src, sc, priors=True, unary_every=10)
        src.Solve(3)
        M = {1}
        lms = sorted(set(int(l) for p, l in zip(sc.obs_pose, sc.obs_lm) if int(p) in M) |
                     set(int(l) for l in range(sc.num_landmarks) if int(sc.lm_ref_pose[l]) in M))
        m = src.Marginalize([1], lms)
        for opts in (pcg_options(), direct_options()):
            h = adjuster.BundleAdjuster(1, 6)
            h.Init(opts)
            scene.populate(h, sc, priors=True, unary_every=10)
            assert h.AddDensePrior(m["pose_ids"], m) == 0
            out.append(h)
    return out


@pytest.mark.parametrize("kind", ["lm1_gn", "lm3_gn", "lm1_dogleg", "lm3_dogleg", "tvs", "calib4", "auto_ordering",
                                  "dense_prior"])
def test_class_with_pcg_tracks_the_direct_solver(kind):
    """Eight Solve(1) calls with Options::reduced_solver = Pcg at 1e-10 against the direct solver from the same start.
    Steps 1-3: equal result codes, converged, proj_error and delta_norm within the project's 1e-6 parity bar; after
    step 8 the states agree to _state_close's 1e-8 and proj_error to 1e-8 relative."""
    import test_gpu_parity as tp
    p, d = _class_pair(kind)
    for it in range(8):
        p.Solve(1)
        d.Solve(1)
        sp, sd = p.summary(), d.summary()
        st = p.GetPcgStats()
        print("%s step %d: result %d / %d, pcg iterations %s, proj_error %.10e / %.10e" % (
            kind, it + 1, sp.result, sd.result, st and st["iterations"], sp.proj_error, sd.proj_error))
        assert d.GetPcgStats() is None
        if it < 3:
            assert sp.result == sd.result, it
            assert st is not None and st["converged"] == 1, (it, st)
            assert abs(sp.proj_error - sd.proj_error) <= 1e-6 * sd.proj_error, it
            assert abs(sp.delta_norm - sd.delta_norm) <= 1e-6 * max(sd.delta_norm, 1e-12), it
    tp._state_close(d, p)
    assert rel_err(p.landmarks(), d.landmarks()) < 1e-8
    assert abs(p.summary().proj_error - d.summary().proj_error) <= 1e-8 * d.summary().proj_error


def _vi_window(opts):
    sc = scene.make_scene(30, 300, 6, lm_dim=1, seed=3, outlier_frac=0.0)
    scene.add_inertial(sc, period=60.0 * 30 / 100.0, seed=3)
    b = adjuster.BundleAdjuster(1, 15)
    b.Init(opts)
    scene.populate(b, sc, imu=True, priors=True, unary_every=10)
    return b


def test_visual_inertial_window_returns_and_the_engine_stays_sound():
    """PoseSize 15, dogleg, 30 poses: cond(S) reaches 1e14 on such windows, CG may stall.  Every Solve(1) returns
    with a result that is not SolverError (ba_hip_solve_gn gave 0 or BA_HIP_FACTORIZATION_ERROR); an engine that ran
    PCG and is switched to DIRECT then gives the bits of an engine that never ran PCG, step after step.
    Measured: all eight steps ran into max_iterations = n = 450 with converged = 0, recurrence
    residual 5.8e-6 .. 2.8; results Success, Success, then ErrorChangeBelowThreshold."""
    o = adjuster.default_options()
    o.reduced_solver = 1
    o.pcg_tolerance = 1e-8
    a = _vi_window(o)
    for it in range(8):
        a.Solve(1)
        s, st = a.summary(), a.GetPcgStats()
        assert adjuster.RESULT_NAMES[s.result] != "SolverError", it
        print("VI window step %d: result %s, pcg %s" % (it + 1, adjuster.RESULT_NAMES[s.result], st and {
            k: st[k] for k in ("iterations", "converged", "residual_replacements", "breakdown", "rel_residual_true",
                               "rel_residual_recurrence")}))
    engines = []
    keep = []
    for solver in (1, 0):
        o = adjuster.default_options()
        o.reduced_solver = solver
        o.pcg_tolerance = 1e-8
        o.apply_results = 0          # the state stays at the start: both engines hold the same problem
        w = _vi_window(o)
        w.Solve(1)
        assert (w.GetPcgStats() is not None) == (solver == 1)
        keep.append(w)
        engines.append(w.engine())
    engines[0].set_reduced_solver(hipapi.SOLVER_DIRECT)
    for e in engines:
        e.begin_solve()
    for it in range(3):
        steps = []
        for e in engines:
            e.linearize()
            rc = e.solve_gn()
            steps.append((rc,) + tuple(e.get_delta_gn()))
            e.compose_step(0.0, 1.0)
            e.apply_step()
        assert steps[0][0] == steps[1][0]
        assert np.array_equal(steps[0][1], steps[1][1]) and np.array_equal(steps[0][2], steps[1][2]), it
    for e in engines:
        e.end_solve()


def test_three_lap_route_too_large_to_download():
    """scene.make_revisit_scene(6000, 120000, 3, 40, 0.3) in natural order, n = 35 988, rel_tolerance 1e-8:
    converged, and ba_hip_check_solve's residual (formed on the device by the dense two-pass product) confirms it;
    1e-9 is what test_config3_full_size_properties grants that tap as its own evaluation noise."""
    P = 6000
    sc = scene.make_revisit_scene(P, 120000, 3, 40, 0.3)
    pa = np.ones(P, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    eng = _engine(sc, pa, revisit=True)
    n = eng.num_pose_params()
    assert n == 35988
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8, max_iterations=n)
    eng.linearize()
    assert eng.solve_gn() == 0
    st = eng.pcg_stats()
    assert st["converged"] == 1, st
    res, rhs = eng.check_solve()
    print("3-lap route n = %d: %d iterations, solve %.2f ms, %.1f us per product (%.2f TB/s), %d tiles, residual %.2e / %.2e"
          % (n, st["iterations"], st["solve_ms"], 1e3 * st["spmv_ms"], st["bytes_read_per_spmv"] / max(st["spmv_ms"], 1e-9) / 1e9,
             st["tiles_read_per_spmv"], st["rel_residual_true"], res / rhs))
    assert rhs > 0 and res / rhs <= 1e-8 + 1e-9, (res, rhs)
    with pytest.raises(hipapi.HipError, match="PCG"):
        eng.compute_marginals()
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.linearize()
    assert eng.solve_gn() == 0
    print("3-lap route: direct solve on the same engine %.2f ms" % eng.get_timers()["solve"])
    eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable():
    from ba_amd import sharding
    sc = scene.make_scene(30, 60, 5, lm_dim=1, seed=7)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    # marginals after a PCG solve
    eng = hipapi.Engine(1, 6)
    eng.set_calibration(0, True)
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::sc.obs_per_landmark + 1] = False
    pa2 = pa.copy()
    pa2[::3] = 0
    eng.set_cameras(sc.cam_params, [0.01, -0.02, 0.03, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa2)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    with pytest.raises(hipapi.HipError, match="did not run the PCG solver"):
        eng.pcg_stats()
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-10)
    eng.linearize()
    assert eng.solve_gn() == 0 and eng.pcg_stats()["converged"] == 1
    x_pcg = eng.get_delta_gn()[0]
    for call in (eng.compute_marginals, lambda: eng.pose_marginals([5]), eng.get_calibration_marginals,
                 eng.calibration_block_marginals):
        with pytest.raises(hipapi.HipError, match="PCG"):
            call()
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.linearize()
    assert eng.solve_gn() == 0
    assert rel_err(x_pcg, eng.get_delta_gn()[0]) < 1e-8
    eng.compute_marginals()
    assert np.all(np.isfinite(eng.get_calibration_marginals()))
    with pytest.raises(hipapi.HipError, match="unknown mode"):
        eng._chk(eng.L.ba_hip_set_reduced_solver(eng.h, 7, None))
    eng.close()
    # sharded engines, both call orders
    ar = sharding.ThreadAllReduce(2)
    eng = hipapi.Engine(1, 6)
    eng.set_allreduce(ar.hook(0), 0, 2)
    with pytest.raises(hipapi.HipError, match="sharded"):
        eng.set_reduced_solver(hipapi.SOLVER_PCG)
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.close()
    eng = hipapi.Engine(1, 6)
    eng.set_reduced_solver(hipapi.SOLVER_PCG)
    with pytest.raises(hipapi.HipError, match="direct reduced solver"):
        eng.set_allreduce(ar.hook(0), 0, 2)
    with pytest.raises(hipapi.HipError, match="direct reduced solver"):
        eng.set_collectives(lambda op, ptr, count, root: 0)
    with pytest.raises(hipapi.HipError, match="direct reduced solver"):
        eng.comm_init(hipapi.Engine.comm_unique_id(), 0, 1)
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.comm_init(hipapi.Engine.comm_unique_id(), 0, 1)    # a single-rank communicator
    with pytest.raises(hipapi.HipError, match="sharded"):
        eng.set_reduced_solver(hipapi.SOLVER_PCG)
    eng.comm_destroy()
    eng.close()
    # ... and the engine behind a refused call still solves
    eng = _engine(sc, pa)
    eng.set_reduced_solver(hipapi.SOLVER_PCG)
    with pytest.raises(hipapi.HipError, match="direct reduced solver"):
        eng.set_allreduce(ar.hook(0), 0, 2)
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    eng.linearize()
    assert eng.solve_gn() == 0
    eng.close()


def test_class_refuses_pcg_on_a_communicator(capfd):
    sc = scene.make_scene(24, 30, 4, lm_dim=1, seed=5)
    a = adjuster.BundleAdjuster(1, 6)
    a.Init(pcg_options())
    fill(a, sc)
    a.set_communicator(hipapi.Engine.comm_unique_id(), 0, 1)
    a.Solve(1)
    assert adjuster.RESULT_NAMES[a.summary().result] == "SolverError"
    assert "reduced_solver = Pcg is not available" in capfd.readouterr().err


def test_demo_application_with_pcg():
    import subprocess
    exe = os.path.join(ROOT, "ba_amd", "lib", "visual_ba_demo")
    runs = [subprocess.run([exe] + extra, capture_output=True, text=True, timeout=120) for extra in ([], ["--pcg", "1e-10"])]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
    assert "step 1: pcg iterations" in runs[1].stdout and "converged 1" in runs[1].stdout
    print(runs[1].stdout)
