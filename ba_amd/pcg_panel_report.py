"""Panel PCG (ba_hip_pcg_panel_solve_system) against the single-column PCG solve of the same system.

    python -m ba_amd.pcg_panel_report [--scenes window200,configs1,revisit6000[,configs3]] [--columns 1,6,64,512]
                                      [--tolerances 1e-6,1e-8] [--out profiles/pcg_panel_report.jsonl]

For every scene and tolerance: one engine linearises once and ba_hip_solve_gn solves the system with the PCG solver
(twice: the second solve finds its plans and buffers; its solve_ms is `single_ms`, the time of one single-column
solve).  Then, on the S that solve leaves in A, one panel solve per column count m (twice, the second is reported):
column 0 is the right-hand side of the Gauss-Newton step, the others are random.  One JSON line per (scene,
tolerance, m): passes, the largest iteration count, solve_ms, the time of one product Q = S P, the bytes and the flops
of a product divided by it, and ratio = solve_ms / (m * single_ms): below 1 the panel beats m single-column solves.
Where a direct solve is affordable (every scene but configs3) a second engine factorises the same system and one more
line gives the error of the joint covariance of six poses (36 unit columns, ba_hip_get_joint_marginals_pcg) against
ba_hip_get_joint_marginals, relative in the 2-norm.  The lines are APPENDED to --out."""
import argparse
import json
import os

import numpy as np

from ba_amd import hipapi
from ba_amd.pcg_report import SCENES, make_engine

COLUMNS = (1, 6, 64, 512)
TOLERANCES = (1e-6, 1e-8)
DIRECT_AFFORDABLE = ("window200", "configs1", "revisit6000")


def run_scene(name, sc, columns=COLUMNS, tolerances=TOLERANCES):
    eng = make_engine(sc)
    ss = eng.structure_stats()
    n = int(eng.num_pose_params())
    base = {"scene": name, "poses": sc.num_poses, "n": n, "tiles_S": ss["tiles_S"], "tiles_L": ss["tiles_L"]}
    rng = np.random.default_rng(1)
    pa = np.ones(sc.num_poses, dtype=bool)
    pa[sc.anchor_poses] = False
    act = np.nonzero(pa)[0]
    six = [int(act[i]) for i in np.linspace(0, len(act) - 1, 6).astype(int)]
    rows = []
    for tol in tolerances:
        eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=tol)
        eng.linearize()
        eng.solve_gn()
        eng.linearize()
        rc = eng.solve_gn()
        st = eng.pcg_stats()
        single = dict(single_rc=rc, single_ms=st["solve_ms"], single_iterations=st["iterations"], single_converged=st["converged"],
                      single_spmv_ms=st["spmv_ms"])
        b = eng.get_rhs()[0]
        for m in columns:
            B = rng.standard_normal((n, m)) * np.linalg.norm(b) / np.sqrt(n)
            B[:, 0] = b
            eng.pcg_panel_solve_system(B, tol)
            X, prc = eng.pcg_panel_solve_system(B, tol)
            ps = eng.pcg_panel_stats()
            col = eng.pcg_panel_columns(m)
            spmm = max(ps["spmm_ms"], 1e-12)
            rows.append(dict(base, rel_tolerance=tol, columns=m, rc=prc, passes=ps["passes"],
                             max_iterations=int(col["iterations"].max()), iterations_column0=int(col["iterations"][0]),
                             converged=ps["converged"], capped=ps["capped"], broken_down=ps["broken_down"],
                             max_rel_residual_true=ps["max_rel_residual_true"], solve_ms=ps["solve_ms"], spmm_ms=ps["spmm_ms"],
                             spmm_TB_per_s=ps["bytes_read_per_product"] / spmm / 1e9,
                             spmm_TFLOP_per_s=ps["tile_products_per_pass"] * 2.0 * 64 ** 3 / spmm / 1e9,
                             tile_products_per_pass=ps["tile_products_per_pass"], workspace_bytes=ps["workspace_bytes"],
                             ratio_to_m_single_solves=ps["solve_ms"] / (m * st["solve_ms"]), **single))
        if name in DIRECT_AFFORDABLE:
            G = eng.joint_marginals_pcg(six, rel_tolerance=tol)
            ps = eng.pcg_panel_stats()
            ref = make_engine(sc)
            ref.linearize()
            if ref.solve_gn() != 0:
                raise RuntimeError("direct solve failed")
            D = ref.joint_marginals(six)
            ref.end_solve()
            ref.close()
            rows.append(dict(base, rel_tolerance=tol, columns=36, joint_poses=six, passes=ps["passes"], solve_ms=ps["solve_ms"],
                             converged=ps["converged"], joint_cov_rel_error_2norm=float(np.linalg.norm(G - D, 2) / np.linalg.norm(D, 2)),
                             **single))
    eng.end_solve()
    eng.close()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="window200,configs1,revisit6000")
    ap.add_argument("--columns", default=",".join("%d" % m for m in COLUMNS))
    ap.add_argument("--tolerances", default=",".join("%g" % t for t in TOLERANCES))
    ap.add_argument("--out", default=os.path.join("profiles", "pcg_panel_report.jsonl"))
    a = ap.parse_args(argv)
    columns = [int(m) for m in a.columns.split(",") if m]
    tolerances = [float(t) for t in a.tolerances.split(",") if t]
    for name in a.scenes.split(","):
        rows = run_scene(name, SCENES[name](), columns, tolerances)
        for r in rows:
            print(json.dumps(r), flush=True)
        if a.out:   # scene by scene: a long run leaves what it finished
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
