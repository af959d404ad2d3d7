"""Cost and accuracy of the solves with the kept factor (ba_hip_factor_solve) and of the weakest modes built on
them (ba_hip_get_weakest_modes) on the scenes of DESIGN.md section 19.

    python -m ba_amd.modes_report [--scenes window200,config1] [--columns 1,64,512] [--modes 1,6,16]
                                  [--out profiles/modes_report.jsonl]

One JSON line per scene and column count m: the device times of the forward and the backward pass
(ba_hip_get_factor_solve_stats; the second of two requests, after the workspace is allocated) and the wall time of
the whole call with its two transfers, beside solve_ms of the direct solve of the same iteration, the levels and the
tile products of the plan, and the error against numpy.linalg.solve on the downloaded S (relative to the largest
entry of the reference).  Then one line per scene and k: iterations, converged pairs, the host-clock times of the
solves and of the orthonormalisation (ba_hip_get_mode_stats), the wall time of the call, and the largest relative
error of the eigenvalues against numpy.linalg.eigh."""
import argparse
import json
import os
import time

import numpy as np

from ba_amd.marginals_report import SCENES, build


def _sym(S):
    return np.where(S == 0.0, S.T, S)


def run(name, sc, mode, columns, ks):
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    eng = build(sc, pa, mode, True)
    for it in range(2):  # one iteration to warm up, then the measured one (left factorised)
        eng.linearize()
        if eng.solve_gn() != 0:
            raise RuntimeError("solve failed")
        if it == 0:
            eng.compose_step(0.0, 1.0)
            eng.apply_step()
    solve_ms = eng.get_timers()["solve"]
    n = eng.num_pose_params() + eng.num_calib_params()
    S = _sym(eng.get_S())
    w = np.linalg.eigvalsh(S)
    w = w[np.argsort(np.abs(w))]
    base = {"scene": name, "n": int(n), "solve_gn_ms": float(solve_ms), "cond_S": float(np.abs(w).max() / np.abs(w).min())}
    rng = np.random.default_rng(0)
    for m in columns:
        B = rng.standard_normal((n, m))
        eng.factor_solve(B)  # allocates the workspace
        t0 = time.perf_counter()
        X = eng.factor_solve(B)
        wall_ms = (time.perf_counter() - t0) * 1e3
        st = eng.factor_solve_stats()
        want = np.linalg.solve(S, B)
        row = dict(base, kind="factor_solve", call_wall_ms=wall_ms,
                   rel_err_vs_numpy_solve=float(np.abs(X - want).max() / np.abs(want).max()))
        row.update({k: (int(v) if isinstance(v, int) else float(v)) for k, v in st.items()})
        row["device_ms_over_solve_gn"] = (row["forward_ms"] + row["backward_ms"]) / max(solve_ms, 1e-9)
        yield row
    for k in ks:
        eng.weakest_modes(k)
        t0 = time.perf_counter()
        lam, _ = eng.weakest_modes(k)
        wall_ms = (time.perf_counter() - t0) * 1e3
        st = eng.mode_stats()
        row = dict(base, kind="weakest_modes", k=int(k), call_wall_ms=wall_ms, lambda_1=float(lam[0]),
                   rel_err_vs_numpy_eigh=float(np.max(np.abs(lam - w[:k]) / np.abs(lam))))
        row.update({k2: (int(v) if isinstance(v, int) else float(v)) for k2, v in st.items()})
        yield row
    eng.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="window200,config1")
    ap.add_argument("--columns", default="1,64,512")
    ap.add_argument("--modes", default="1,6,16")
    ap.add_argument("--out", default=os.path.join("profiles", "modes_report.jsonl"))
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for key in a.scenes.split(","):
            name, sc, mode = SCENES[key]()
            for row in run(name, sc, mode, [int(x) for x in a.columns.split(",")], [int(x) for x in a.modes.split(",")]):
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
