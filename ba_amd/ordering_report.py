"""Natural vs AUTO pose ordering on a multi-lap route (scene.make_revisit_scene).

    python -m ba_amd.ordering_report --poses 6000 --laps 3 [--landmarks N] [--window W] [--revisit F] [--iters K]

Builds the scene, finalizes one engine with BA_HIP_ORDER_NATURAL and one with BA_HIP_ORDER_AUTO, runs a
few Gauss-Newton iterations of each, and prints one JSON line per mode: the factor's tile products, the
solve time of the iterations (ba_hip_get_timers), the finalize time, the ordering statistics and the
largest relative difference of the pose steps between the two modes."""
import argparse
import json
import time

import numpy as np

from ba_amd import hipapi, scene


def run_mode(sc, pa, mode, iters):
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
    eng.set_pose_ordering(mode)
    t0 = time.perf_counter()
    eng.finalize()
    fin_ms = 1e3 * (time.perf_counter() - t0)
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    steps = []
    t_solve0 = eng.get_timers()["solve"]
    for _ in range(iters):
        eng.linearize()
        rc = eng.solve_gn()
        if rc != 0:
            raise RuntimeError("solve failed (%d)" % rc)
        steps.append(eng.get_delta_gn()[0].copy())
        eng.compose_step(0.0, 1.0)
        eng.apply_step()
    solve_ms = eng.get_timers()["solve"] - t_solve0
    eng.end_solve()
    _, ost = eng.get_pose_ordering()
    res = {"mode": {0: "natural", 1: "auto"}[mode], "poses": sc.num_poses, "laps": sc.laps,
           "factor_tile_products": eng.structure_stats()["factor_tile_products"],
           "solve_ms_per_iter": solve_ms / max(iters, 1), "finalize_ms": fin_ms, "ordering": ost}
    eng.close()
    return res, steps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--poses", type=int, default=3000)
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--landmarks", type=int, default=0, help="default: 20 per pose")
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--revisit", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    L = a.landmarks or 20 * a.poses
    sc = scene.make_revisit_scene(a.poses, L, a.laps, a.window, a.revisit, seed=a.seed)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    out = {}
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO):
        out[mode] = run_mode(sc, pa, mode, a.iters)
    diff = max(float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300))
               for x, y in zip(out[hipapi.ORDER_AUTO][1], out[hipapi.ORDER_NATURAL][1]))
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO):
        r = out[mode][0]
        r["landmarks"], r["window"], r["revisit_frac"], r["iters"] = L, a.window, a.revisit, a.iters
        r["max_rel_delta_p_diff"] = diff
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
