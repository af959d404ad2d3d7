"""Direct (tile-sparse LDL^T) against iterative (block-Jacobi PCG) solve of the reduced camera system.

    python -m ba_amd.pcg_report [--scenes window200,configs1,revisit6000[,configs3][,vi30]] [--coarse G[,G...]]
                                [--tolerances 1e-6,1e-8] [--out profiles/pcg_report.jsonl]

For every scene: one engine linearises once and solves the same system with the direct solver and with PCG at
rel_tolerance 1e-2, 1e-4, 1e-6, 1e-8 (ba_hip_set_reduced_solver is not structural).  One JSON line per (scene,
solver): the direct solve's time (ba_hip_get_timers), and for PCG the iterations, solve_ms, the time of one product
q = S p, bytes_read_per_spmv divided by it, the relative difference of the pose step from the direct one, and the
projection error after 5 Gauss-Newton iterations with that solver from the same start (a fresh engine per run).
--coarse adds, beside every PCG row, one row per aggregate size G for the two-level preconditioner
(ba_hip_pcg_options.coarse_aggregate): the same figures plus the coarse space, its setup_ms and apply_ms.  The scene
vi30 is the 30-pose visual-inertial window (PoseSize 15, dogleg) through the class: five Solve(1) calls per solver.
The lines are APPENDED to --out: a rerun adds its rows behind the earlier ones (each line names its scene, solver,
tolerance and coarse_aggregate); delete the file first to replace them."""
import argparse
import json
import os

import numpy as np

from ba_amd import hipapi, scene

TOLERANCES = (1e-2, 1e-4, 1e-6, 1e-8)
SCENES = {
    "window200": lambda: scene.make_scene(200, 20000, 10, lm_dim=1, seed=2),
    "configs1": lambda: scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2),
    "revisit6000": lambda: scene.make_revisit_scene(6000, 120000, 3, 40, 0.3),
    "configs3": lambda: scene.make_scene(10000, 1000000, 10, lm_dim=1, seed=2),
}


def make_engine(sc):
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    eng = hipapi.Engine(1, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    eng.set_options(o)
    keep = np.r_[False, np.diff(sc.obs_lm) == 0]  # the reference frame's observation defines the landmark
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    return eng


def select(eng, tol, coarse=0):
    if tol is None:
        eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    else:
        eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=tol, coarse_aggregate=coarse)


def five_iterations(sc, tol, iters=5, coarse=0):
    eng = make_engine(sc)
    select(eng, tol, coarse)
    solve_ms, its = 0.0, []
    for _ in range(iters):
        eng.linearize()
        if eng.solve_gn() != 0:
            break
        solve_ms += eng.get_timers()["solve"]
        if tol is not None:
            its.append(eng.pcg_stats()["iterations"])
        eng.compose_step(0.0, 1.0)
        eng.apply_step()
    err = eng.eval_residuals().proj_error
    eng.end_solve()
    eng.close()
    return err, solve_ms, its


def run_vi_window(tolerances, coarse):
    """scene.make_scene(30, 300, 6) with inertial residuals, PoseSize 15, dogleg, through ba::BundleAdjuster"""
    from ba_amd import adjuster
    rows = []
    for tol, g in [(None, 0)] + [(t, g) for t in tolerances for g in [0] + list(coarse)]:
        sc = scene.make_scene(30, 300, 6, lm_dim=1, seed=3, outlier_frac=0.0)
        scene.add_inertial(sc, period=60.0 * 30 / 100.0, seed=3)
        o = adjuster.default_options()
        o.reduced_solver = 0 if tol is None else 1
        o.pcg_tolerance = tol or 1e-6
        o.pcg_coarse_aggregate = g
        b = adjuster.BundleAdjuster(1, 15)
        b.Init(o)
        scene.populate(b, sc, imu=True, priors=True, unary_every=10)
        its, conv, ms, results = [], [], 0.0, []
        for _ in range(5):
            b.Solve(1)
            st = b.GetPcgStats()
            ms += b.timers()["solve"]
            results.append(adjuster.RESULT_NAMES[b.summary().result])
            if st:
                its.append(st["iterations"])
                conv.append(st["converged"])
        s = b.summary()
        row = {"scene": "vi30", "poses": 30, "n": 450, "solver": "direct" if tol is None else "pcg", "results": results,
               "solve_ms_5_iterations": ms, "proj_error_after_5": s.proj_error, "inertial_error_after_5": s.inertial_error}
        if tol is not None:
            row.update(rel_tolerance=tol, coarse_aggregate=g, iterations_5=its, converged_5=conv)
            cst = b.GetPcgCoarseStats()
            if cst:
                row.update({k: cst[k] for k in ("aggregate_used", "coarse_unknowns", "setup_ms", "apply_ms")})
        rows.append(row)
    return rows


def run_scene(name, sc, tolerances=TOLERANCES, coarse=()):
    eng = make_engine(sc)
    ss = eng.structure_stats()
    base = {"scene": name, "poses": sc.num_poses, "n": int(eng.num_pose_params()), "tiles_S": ss["tiles_S"], "tiles_L": ss["tiles_L"]}
    select(eng, None)
    eng.linearize()
    if eng.solve_gn() != 0:
        raise RuntimeError("direct solve failed")
    eng.linearize()           # the second solve of the same system: plans and buffers exist
    eng.solve_gn()
    direct_ms = eng.get_timers()["solve"]
    dp = eng.get_delta_gn()[0].copy()
    rows = []
    err, ms5, _ = five_iterations(sc, None)
    rows.append(dict(base, solver="direct", solve_ms=direct_ms, proj_error_after_5=err, solve_ms_5_iterations=ms5))
    for tol, g in [(t, g) for t in tolerances for g in [0] + list(coarse)]:
        select(eng, tol, g)
        eng.linearize()
        eng.solve_gn()
        eng.linearize()
        rc = eng.solve_gn()
        st = eng.pcg_stats()
        x = eng.get_delta_gn()[0]
        err, ms5, its = five_iterations(sc, tol, coarse=g)
        extra = {}
        if g:
            cst = eng.pcg_coarse_stats()
            extra = {k: cst[k] for k in ("aggregate_used", "coarse_unknowns", "aggregates", "setup_ms", "apply_ms", "coarse_bytes")}
        rows.append(dict(base, solver="pcg", rel_tolerance=tol, coarse_aggregate=g, **extra, rc=rc, iterations=st["iterations"], converged=st["converged"],
                         residual_replacements=st["residual_replacements"], rel_residual_true=st["rel_residual_true"],
                         solve_ms=st["solve_ms"], engine_solve_ms=eng.get_timers()["solve"], precond_ms=st["precond_ms"],
                         spmv_ms=st["spmv_ms"], bytes_read_per_spmv=st["bytes_read_per_spmv"],
                         spmv_TB_per_s=st["bytes_read_per_spmv"] / max(st["spmv_ms"], 1e-12) / 1e9,
                         direct_solve_ms=direct_ms, rel_delta_p_vs_direct=float(np.linalg.norm(x - dp) / np.linalg.norm(dp)),
                         proj_error_after_5=err, solve_ms_5_iterations=ms5, iterations_5=its))
    eng.end_solve()
    eng.close()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="window200,configs1,revisit6000")
    ap.add_argument("--coarse", default="", help="aggregate sizes of the two-level preconditioner, e.g. 10,4")
    ap.add_argument("--tolerances", default=",".join("%g" % t for t in TOLERANCES))
    ap.add_argument("--out", default=os.path.join("profiles", "pcg_report.jsonl"))
    a = ap.parse_args(argv)
    coarse = [int(g) for g in a.coarse.split(",") if g]
    tolerances = [float(t) for t in a.tolerances.split(",") if t]
    lines = []
    for name in a.scenes.split(","):
        rows = run_vi_window(tolerances, coarse) if name == "vi30" else run_scene(name, SCENES[name](), tolerances, coarse)
        for r in rows:
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
