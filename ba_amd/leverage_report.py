"""Cost and sanity of the projection leverages (ba_hip_get_projection_leverages: the 2 x 2 hat blocks of every
projection residual from the selected inverse) on the scenes of DESIGN.md section 15.

    python -m ba_amd.leverage_report [--scenes window50,window200,config1] [--out profiles/leverage_report.jsonl]

One JSON line per scene, printed and written to --out (the file is replaced): the device time of the all-residuals pass
(ba_hip_get_leverage_stats) beside the selected inverse's and the landmark pass's of the same factor in the same
process (ba_hip_get_marginal_stats) — the landmark pass does the same k^2 block reads per landmark and is the
yardstick —, the blocks of Sigma read, the sum of the traces against the number of unknowns the residuals touch, and
the histogram of the redundancy numbers 2 - tr H_aa in ten bins over [0, 2]."""
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


SCENES = {
    "window50": lambda: ("window50", scene.make_scene(50, 2000, 6, lm_dim=1, seed=1)),
    "window200": lambda: ("window200", scene.make_scene(200, 8000, 6, lm_dim=1, seed=1)),
    "config1": lambda: ("configs[1]", scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2)),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--out", default=os.path.join("profiles", "leverage_report.jsonl"))
    a = ap.parse_args(argv)
    lines = []
    for key in a.scenes.split(","):
        name, sc = SCENES[key]()
        lines.append(json.dumps(run(name, sc)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
