"""Cost and sanity of the projection leverages (ba_hip_get_projection_leverages: the 2 x 2 hat blocks of every
projection residual from the selected inverse) on the scenes of DESIGN.md section 15.

    python -m ba_amd.leverage_report [--scenes window50,window200,config1] [--out profiles/leverage_report.jsonl]

One JSON line per scene, printed and written to --out (the file is replaced): the device time of the all-residuals pass
(ba_hip_get_leverage_stats) beside the selected inverse's and the landmark pass's of the same factor in the same
process (ba_hip_get_marginal_stats) — the landmark pass does the same k^2 block reads per landmark and is the
yardstick —, the blocks of Sigma read, the sum of the traces against the number of unknowns the residuals touch, and
the histogram of the redundancy numbers 2 - tr H_aa in ten bins over [0, 2].

    python -m ba_amd.leverage_report --pose-pose [--scenes ""]

adds one line per window of DESIGN.md section 16 (30- and 100-pose visual-inertial windows, PoseSize 15; the 200-pose
visual window with priors and odometry, PoseSize 6; all through ba::BundleAdjuster): the device time of
ba_hip_get_pose_pose_leverages per residual kind (ba_hip_get_pose_pose_leverage_stats) beside the selected inverse's
and the projection pass's of the same factor, the blocks of Sigma read, and the sum of all leverages (projection
traces included) against the unknowns."""
import argparse
import json
import os

import numpy as np

from ba_amd import hipapi, scene
from ba_amd.marginals_report import build


def run(name, sc):
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    n = int(pa.sum()) * 6
    eng = build(sc, pa, hipapi.ORDER_NATURAL, False)
    # one iteration to warm up, then the measured one (left factorised)
    for it in range(2):
        eng.linearize()
        if eng.solve_gn() != 0:
            raise RuntimeError("solve failed")
        if it == 0:
            eng.compose_step(0.0, 1.0)
            eng.apply_step()
    # first requests allocate the store and load the kernels; the second ones are timed
    eng.landmark_marginals(None)
    eng.projection_leverages()
    eng.landmark_marginals(None)
    h = eng.projection_leverages()
    mst, lst = eng.marginal_stats(), eng.leverage_stats()
    tr = np.trace(h, axis1=1, axis2=2)
    red = 2.0 - tr
    hist, _ = np.histogram(red, bins=10, range=(0.0, 2.0))
    res = {"scene": name, "poses": sc.num_poses, "landmarks": sc.num_landmarks, "n": n, "residuals": int(lst["residuals"]),
           "selinv_ms": float(mst["selinv_ms"]), "landmark_ms": float(mst["landmark_ms"]),
           "device_ms": float(lst["device_ms"]), "block_reads": int(lst["block_reads"]),
           "leverage_over_landmark": float(lst["device_ms"] / max(mst["landmark_ms"], 1e-9)),
           "sum_trace": float(tr.sum()), "unknowns": n + sc.num_landmarks,
           "redundancy_min": float(red.min()), "redundancy_median": float(np.median(red)),
           "redundancy_max": float(red.max()), "redundancy_hist": [int(c) for c in hist]}
    eng.close()
    return res


def run_pose_pose(name, P, L, inertial):
    """one window through the class: two Gauss-Newton iterations, then every leverage of the last factor"""
    from ba_amd import adjuster
    D = 15 if inertial else 6
    sc = scene.make_scene(P, L, 6, lm_dim=1, seed=1)
    if inertial:
        scene.add_inertial(sc, period=60.0 * P / 100.0)
    o = adjuster.default_options()
    o.use_dogleg = 0
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    h = adjuster.BundleAdjuster(1, D)
    h.Init(o)
    pa = np.ones(P, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    scene.populate(h, sc, active=pa, imu=inertial, priors=True, unary_every=10)
    h.Solve(2)
    if adjuster.RESULT_NAMES[h.summary().result] in ("FactorizationError", "SolverError"):
        raise RuntimeError("solve failed")
    eng = h.engine()
    res = {"scene": name, "poses": P, "landmarks": L, "pose_size": D, "n": int(eng.num_pose_params())}
    total = 0.0
    for rep in range(2):   # first requests allocate the store and load the kernels; the second ones are timed
        proj = eng.projection_leverages()
        res["projection_ms"] = float(eng.leverage_stats()["device_ms"])
        for kind, key in ((hipapi.RES_UNARY, "unary"), (hipapi.RES_BINARY, "binary"), (hipapi.RES_IMU, "inertial")):
            lev = eng.pose_pose_leverages(kind, want=(False, False, True))[2]
            st = eng.pose_pose_leverage_stats()
            res[key] = {"residuals": int(st["residuals"]), "device_ms": float(st["device_ms"]),
                        "sigma_blocks": int(st["sigma_blocks"]), "sum": float(lev.sum()),
                        "median": float(np.median(lev)) if len(lev) else 0.0, "max": float(lev.max()) if len(lev) else 0.0}
    res["selinv_ms"] = float(eng.marginal_stats()["selinv_ms"])
    total = float(np.trace(proj, axis1=1, axis2=2).sum()) + sum(res[k]["sum"] for k in ("unary", "binary", "inertial"))
    res["sum_all_leverages"] = total
    res["unknowns_upper"] = int(eng.num_pose_params()) + int(eng.num_lm_params())   # (masked parameters included)
    return res


POSE_POSE = [("vi_window30", 30, 1200, True), ("vi_window100", 100, 4000, True), ("window200_odometry", 200, 8000, False)]

SCENES = {
    "window50": lambda: ("window50", scene.make_scene(50, 2000, 6, lm_dim=1, seed=1)),
    "window200": lambda: ("window200", scene.make_scene(200, 8000, 6, lm_dim=1, seed=1)),
    "config1": lambda: ("configs[1]", scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2)),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--pose-pose", action="store_true", help="also the pose-pose leverages on the windows of section 16")
    ap.add_argument("--out", default=os.path.join("profiles", "leverage_report.jsonl"))
    a = ap.parse_args(argv)
    lines = []
    for key in [k for k in a.scenes.split(",") if k]:
        name, sc = SCENES[key]()
        lines.append(json.dumps(run(name, sc)))
        print(lines[-1], flush=True)
    if a.pose_pose:
        for w in POSE_POSE:
            lines.append(json.dumps(run_pose_pose(*w)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
