"""Cost and accuracy of the joint covariances of pose sets (ba_hip_get_joint_marginals: forward substitution
over the reach and a Gram product, no selected inverse) on the scenes of DESIGN.md section 14.

    python -m ba_amd.joint_marginals_report [--scenes window200,config1,revisit_natural,revisit_auto]
                                            [--sets 2,8,64] [--out profiles/joint_marginals_report.jsonl]

One JSON line per scene and set of poses (2: the first and the last active pose; 8 and 64: spread evenly over
the trajectory): the columns, the reach tiles, the levels and the tile products of the plan, the device times of
the substitution and of the Gram product (ba_hip_get_joint_marginal_stats; the second of two requests, after the
workspace is allocated), the wall time of the whole call, beside them the device time, the tile products and the
store of the selected inverse of the same factor in the same process (ba_hip_get_marginal_stats, second request),
and where S is small enough to download (n <= 6000) the error against inv(S), relative to the largest entry of
the reference block."""
import argparse
import json
import os
import time

import numpy as np

from ba_amd import hipapi, scene
from ba_amd.marginals_report import SCENES, build


def run(name, sc, mode, sets):
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    act = np.nonzero(pa)[0]
    n = len(act) * 6
    dense = n <= 6000
    eng = build(sc, pa, mode, dense)
    for it in range(2):  # one iteration to warm up, then the measured one (left factorised)
        eng.linearize()
        if eng.solve_gn() != 0:
            raise RuntimeError("solve failed")
        if it == 0:
            eng.compose_step(0.0, 1.0)
            eng.apply_step()
    solve_ms = eng.get_timers()["solve"]
    rows = []
    got = {}
    for k in sets:
        ids = act[[0, -1]] if k == 2 else act[np.linspace(0, len(act) - 1, k).astype(int)]
        eng.joint_marginals(ids)  # allocates the workspace
        t0 = time.perf_counter()
        got[k] = (ids, eng.joint_marginals(ids))
        wall_ms = (time.perf_counter() - t0) * 1e3
        st = eng.joint_marginal_stats()
        row = {"scene": name, "n": n, "order": {0: "natural", 1: "auto"}[mode], "poses": int(k), "solve_gn_ms": solve_ms,
               "call_wall_ms": wall_ms}
        row.update({k2: (int(v) if isinstance(v, int) else float(v)) for k2, v in st.items()})
        rows.append(row)
    # the selected inverse of the same factor, second request
    eng.compute_marginals()
    eng.release_marginals()
    eng.compute_marginals()
    ms = eng.marginal_stats()
    Si = None
    if dense:
        Si = np.linalg.inv(eng.get_S())
        opt = np.full(sc.num_poses, -1, dtype=np.int64)
        opt[act] = np.arange(len(act))
    for row in rows:
        row["selinv_ms"] = float(ms["selinv_ms"])
        row["selinv_tile_products"] = int(ms["tile_products"])
        row["selinv_store_bytes"] = float(ms["store_bytes"])
        row["device_ms_over_selinv"] = (row["solve_ms"] + row["gram_ms"]) / max(ms["selinv_ms"], 1e-9)
        if Si is not None:
            ids, cov = got[row["poses"]]
            r = np.array([opt[p] * 6 + x for p in ids for x in range(6)])
            want = Si[np.ix_(r, r)]
            row["rel_err_vs_inv_S"] = float(np.abs(cov - want).max() / np.abs(want).max())
            row["cross_over_max"] = float(np.abs(cov[:6, -6:]).max() / np.abs(cov).max())
    eng.close()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="window200,config1,revisit_natural,revisit_auto")
    ap.add_argument("--sets", default="2,8,64")
    ap.add_argument("--out", default=os.path.join("profiles", "joint_marginals_report.jsonl"))
    a = ap.parse_args(argv)
    sets = [int(x) for x in a.sets.split(",")]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for key in a.scenes.split(","):
            name, sc, mode = SCENES[key]()
            for row in run(name, sc, mode, sets):
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
