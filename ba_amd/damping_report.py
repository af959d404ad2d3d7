"""Levenberg-Marquardt steps (ba_hip_set_damping) beside undamped Gauss-Newton steps from the same start.

    python -m ba_amd.damping_report [--scenes window200,configs1[,configs3]] [--iterations 6] [--lambda0 1e-4]
                                    [--out profiles/damping_report.jsonl]

For every scene two engines start from the same state.  The undamped one takes plain Gauss-Newton steps (a step that
raises the error is rolled back and the run ends, as Solve() does).  The damped one follows the host loop of
BundleAdjuster::SolveInternal: solve, compose (0, 1), evaluate, apply, evaluate, gain ratio, Nielsen's rule
(ba_hip_damping_update); a rejected step is rolled back and the system linearised again with the larger lambda.  One
JSON line per (scene, mode, iteration): lambda, rho, the error before and after, the rejected inner steps, the
engine's linearise and solve timers, and for the damped run device_ms of the damping kernels (k_damp_poses +
k_damp_terms; k_pose_schur_diag runs on the second stream beside the tile assembly and shows in jtj_schur) and the
range of the damping diagonal.  The lines are APPENDED to --out."""
import argparse
import ctypes
import json
import os

from ba_amd.pcg_report import SCENES, make_engine


def update(eng, lam, nu, rho):
    """Nielsen's rule through the library: (lambda, nu, accepted)"""
    a, b = ctypes.c_double(lam), ctypes.c_double(nu)
    rc = eng._chk(eng.L.ba_hip_damping_update(eng.h, ctypes.byref(a), ctypes.byref(b), ctypes.c_double(rho)), positive_ok=True)
    return a.value, b.value, rc == 1


def timers(eng):
    t = eng.get_timers()
    return {"linearize_ms": t["j_evaluation"] + t["robust_weights"] + t["jtj_schur"], "jtj_schur_ms": t["jtj_schur"],
            "solve_ms": t["solve"] + t["back_substitution"]}


def run_undamped(name, sc, iterations):
    eng = make_engine(sc)
    rows = []
    for it in range(iterations):
        eng.linearize()
        if eng.solve_gn() != 0:
            rows.append({"scene": name, "mode": "gauss_newton", "iteration": it, "result": "FactorizationError"})
            break
        t = timers(eng)
        eng.compose_step(0.0, 1.0)
        pre = eng.eval_residuals().total()
        eng.apply_step()
        post = eng.eval_residuals().total()
        rows.append(dict({"scene": name, "mode": "gauss_newton", "iteration": it, "error_before": pre, "error_after": post,
                          "result": "Success" if post <= pre else "ErrorIncreased"}, **t))
        if post > pre:
            eng.rollback()
            break
    eng.end_solve()
    eng.close()
    return rows


def run_damped(name, sc, iterations, lambda0, max_inner=20):
    eng = make_engine(sc)
    lam, nu = lambda0, 2.0
    rows = []
    for it in range(iterations):
        rejected = 0
        while True:
            eng.set_damping(lam)
            eng.linearize()
            if eng.solve_gn() != 0:
                rows.append({"scene": name, "mode": "levenberg_marquardt", "iteration": it, "result": "FactorizationError"})
                eng.close()
                return rows
            t, terms = timers(eng), eng.damping_terms()
            eng.compose_step(0.0, 1.0)
            pre = eng.eval_residuals().total()
            eng.apply_step()
            post = eng.eval_residuals().total()
            rho = (pre - post) / terms["predicted_decrease"]
            used = lam
            lam, nu, accepted = update(eng, lam, nu, rho)
            if accepted or rejected + 1 >= max_inner:
                break
            eng.rollback()
            rejected += 1
        rows.append(dict({"scene": name, "mode": "levenberg_marquardt", "iteration": it, "lambda": used, "lambda_next": lam, "rho": rho,
                          "error_before": pre, "error_after": post, "rejected": rejected,
                          "result": "Success" if accepted else "ErrorIncreased", "damping_device_ms": terms["device_ms"],
                          "diag_min": terms["diag_min"], "diag_max": terms["diag_max"]}, **t))
        if not accepted:
            eng.rollback()
            break
    eng.set_damping(0.0)
    eng.end_solve()
    eng.close()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="window200,configs1")
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--lambda0", type=float, default=1e-4)
    ap.add_argument("--out", default=os.path.join("profiles", "damping_report.jsonl"))
    a = ap.parse_args(argv)
    lines = []
    for name in a.scenes.split(","):
        sc = SCENES[name]()
        for r in run_undamped(name, sc, a.iterations) + run_damped(name, sc, a.iterations, a.lambda0):
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
