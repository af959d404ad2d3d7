"""Device time of ba_hip_refine_poses beside the Jacobian evaluation of one ba_hip_linearize.

    python -m ba_amd.resection_report [--scenes window200,configs1] [--repeats 3] [--out profiles/resection_report.jsonl]

For every scene one engine: the audit call (write_back = 0, every pose, the defaults) `repeats` times, then the same for
one pose alone (the tracking case: the pose with the most observations), then one writing call, and after it
ba_hip_begin_solve and one ba_hip_linearize for timers.j_evaluation.  One JSON line per (scene, request): device_ms of
every repeat (event-timed: request upload, pose tables, kernels), the counts per status, the mean and largest iteration
count, the observations used and excluded, the largest observation count of a requested pose, and j_evaluation_ms of
the linearisation.  No target is set: the figures say what the call costs next to a kernel family that walks the same
observations once.  The lines are APPENDED to --out."""
import argparse
import json
import os

import numpy as np

from ba_amd import hipapi
from ba_amd.pcg_report import SCENES, make_engine


def run(name, sc, repeats):
    eng = make_engine(sc)
    eng.end_solve()      # make_engine leaves the engine inside a Solve: the refinement runs outside
    rows = []

    def call(request, ids, **kw):
        ms, res, st = [], None, None
        for _ in range(repeats if not kw.get("write_back", 0) else 1):
            res, _, _ = eng.refine_poses(ids, **kw)
            st = eng.pose_refinement_stats()
            ms.append(st["device_ms"])
        rows.append({"scene": name, "request": request, "poses": st["poses"], "observations_used": st["observations_used"],
                     "observations_excluded": st["observations_excluded"], "device_ms": ms, "count": st["count"],
                     "written": st["written"], "iterations_mean": float(res[:, hipapi.RESECT_ITERATIONS].mean()),
                     "iterations_max": int(res[:, hipapi.RESECT_ITERATIONS].max()),
                     "observations_max": int((res[:, hipapi.RESECT_USED] + res[:, hipapi.RESECT_EXCLUDED]).max())})
        return res

    res = call("audit_all", None, write_back=0)
    busiest = int(np.argmax(res[:, hipapi.RESECT_USED]))
    call("audit_one_pose", np.array([busiest], dtype=np.uint32), write_back=0)
    call("write_all", None, write_back=1)
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    eng.linearize()
    j = eng.get_timers()["j_evaluation"]
    for r in rows:
        r["j_evaluation_ms"] = j
    eng.end_solve()
    eng.close()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="window200,configs1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "resection_report.jsonl"))
    a = ap.parse_args(argv)
    lines = []
    for name in a.scenes.split(","):
        for r in run(name, SCENES[name](), a.repeats):
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
