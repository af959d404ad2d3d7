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
the reference block.

    python -m ba_amd.joint_marginals_report --landmarks N [--scenes window200,config1]

measures the mixed call instead (ba_hip_get_joint_state_marginals): the last active pose, the active reference
poses of its landmarks (as many as fit beside the landmark columns) and N landmarks, those the last pose observes
first, then the ones with the highest ids.  One JSON line per scene, APPENDED to the output: the device times of the
seed pass, the right-hand-side pass, the substitution and the Gram product and the wall time of the second of two
requests; the pose-only joint call over the same poses; and the selected inverse plus the landmark pass
(ba_hip_get_landmark_marginals over the same landmarks) of the same factor, second request."""
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


def run_landmarks(name, sc, mode, n_lms):
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    act = np.nonzero(pa)[0]
    eng = build(sc, pa, mode, False)
    for it in range(2):
        eng.linearize()
        if eng.solve_gn() != 0:
            raise RuntimeError("solve failed")
        if it == 0:
            eng.compose_step(0.0, 1.0)
            eng.apply_step()
    last = int(act[-1])
    seen = sorted(set(int(l) for l in sc.obs_lm[sc.obs_pose == last]), reverse=True)
    rest = [l for l in range(sc.num_landmarks - 1, -1, -1) if l not in set(seen)]
    lms = (seen + rest)[:n_lms]
    room = (hipapi.JOINT_MAX_COLUMNS - len(lms)) // 6
    refs = []
    for l in lms:
        p = int(sc.lm_ref_pose[l])
        if pa[p] and p != last and p not in refs:
            refs.append(p)
    poses = ([last] + refs)[:max(room, 1)]
    eng.joint_state_marginals(poses, lms)  # allocates the workspace
    t0 = time.perf_counter()
    cov = eng.joint_state_marginals(poses, lms)
    wall_ms = (time.perf_counter() - t0) * 1e3
    js, ss = eng.joint_marginal_stats(), eng.joint_state_stats()
    eng.joint_marginals(poses)
    t0 = time.perf_counter()
    eng.joint_marginals(poses)
    pose_wall_ms = (time.perf_counter() - t0) * 1e3
    ps = eng.joint_marginal_stats()
    eng.compute_marginals()
    eng.release_marginals()
    eng.compute_marginals()
    eng.landmark_marginals(lms)
    ms = eng.marginal_stats()
    d = np.sqrt(np.diag(cov))
    c0 = 6 * len(poses)
    corr = cov / np.outer(d, d)
    row = {"scene": name, "n": int(len(act) * 6), "order": {0: "natural", 1: "auto"}[mode], "kind": "joint_state",
           "poses": len(poses), "landmarks": len(lms), "call_wall_ms": wall_ms,
           "max_pose_landmark_correlation": float(np.abs(corr[:c0, c0:]).max()),
           "pose_only_solve_ms": float(ps["solve_ms"]), "pose_only_gram_ms": float(ps["gram_ms"]),
           "pose_only_reach_tiles": int(ps["reach_tiles"]), "pose_only_call_wall_ms": pose_wall_ms,
           "selinv_ms": float(ms["selinv_ms"]), "selinv_landmark_ms": float(ms["landmark_ms"])}
    row.update({k: (int(v) if isinstance(v, int) else float(v)) for k, v in list(js.items()) + list(ss.items())})
    row["device_ms_over_selinv"] = (row["seed_ms"] + row["rhs_ms"] + row["solve_ms"] + row["gram_ms"]) / \
        max(ms["selinv_ms"] + ms["landmark_ms"], 1e-9)
    eng.close()
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="window200,config1,revisit_natural,revisit_auto")
    ap.add_argument("--sets", default="2,8,64")
    ap.add_argument("--landmarks", type=int, default=0, help="measure the mixed call with this many landmarks (appends)")
    ap.add_argument("--out", default=os.path.join("profiles", "joint_marginals_report.jsonl"))
    a = ap.parse_args(argv)
    sets = [int(x) for x in a.sets.split(",")]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    if a.landmarks:
        with open(a.out, "a") as f:
            for key in a.scenes.split(","):
                name, sc, mode = SCENES[key]()
                line = json.dumps(run_landmarks(name, sc, mode, a.landmarks))
                print(line, flush=True)
                f.write(line + "\n")
        return
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
