"""Cost and accuracy of the marginal covariances (ba_hip_compute_marginals: selected inverse of the reduced
system, then the landmark pass) on the scenes of DESIGN.md section 11.

    python -m ba_amd.marginals_report [--scenes window50,window200,config1,revisit_natural,revisit_auto]

One JSON line per scene: the solve time of the iteration (ba_hip_get_timers), the device time of the selected
inverse and of the landmark pass over every active landmark (ba_hip_get_marginal_stats; the second of two
requests, after the store is allocated), the tile products of the selected inverse and of the factorisation,
the bytes of the store, the number of launch levels, and where a dense inverse is affordable (n <= 3000) the
largest relative error of a pose block against inv(S)."""
import argparse
import json

import numpy as np

from ba_amd import hipapi, scene


def build(sc, pa, mode, keep_S):
    eng = hipapi.Engine(1, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.keep_reduced_system = int(keep_S)
    eng.set_options(o)
    keep = np.r_[False, np.diff(sc.obs_lm) == 0]  # the reference frame's observation defines the landmark
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    eng.set_pose_ordering(mode)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    return eng


def run(name, sc, mode=hipapi.ORDER_NATURAL):
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    n = int(pa.sum()) * 6
    dense = n <= 3000
    eng = build(sc, pa, mode, dense)
    # one iteration to warm up, then the measured one (left factorised)
    for it in range(2):
        eng.linearize()
        if eng.solve_gn() != 0:
            raise RuntimeError("solve failed")
        if it == 0:
            eng.compose_step(0.0, 1.0)
            eng.apply_step()
    solve_ms = eng.get_timers()["solve"]
    eng.compute_marginals()
    act = np.nonzero(pa)[0]
    cov = eng.pose_marginals(act)
    lm = eng.landmark_marginals(None)
    # second request: the store exists, the device times are the kernels' own
    eng.release_marginals()
    eng.compute_marginals()
    eng.landmark_marginals(None)
    st = eng.marginal_stats()
    res = {"scene": name, "poses": sc.num_poses, "landmarks": sc.num_landmarks, "n": n,
           "order": {0: "natural", 1: "auto"}[mode], "solve_ms": solve_ms}
    res.update({k: (int(v) if isinstance(v, int) else float(v)) for k, v in st.items()})
    res["selinv_over_solve"] = st["selinv_ms"] / max(solve_ms, 1e-9)
    res["products_over_factor"] = st["tile_products"] / max(st["factor_tile_products"], 1)
    res["pose_sigma_t_median"] = float(np.median(np.sqrt(cov[:, 0, 0])))
    res["landmark_sigma_median"] = float(np.median(np.sqrt(np.maximum(lm[:, 0, 0], 0))))
    if dense:
        S = eng.get_S()
        Si = np.linalg.inv(S)
        err = 0.0
        for q, p in enumerate(act):
            r = q * 6
            w = Si[r:r + 6, r:r + 6]
            err = max(err, float(np.abs(cov[q] - w).max() / np.abs(w).max()))
        res["max_pose_block_rel_err"] = err
        res["cond_S"] = float(np.linalg.cond(S))
    eng.close()
    return res


SCENES = {
    "window50": lambda: ("window50", scene.make_scene(50, 2000, 6, lm_dim=1, seed=1), hipapi.ORDER_NATURAL),
    "window200": lambda: ("window200", scene.make_scene(200, 8000, 6, lm_dim=1, seed=1), hipapi.ORDER_NATURAL),
    "config1": lambda: ("configs[1]", scene.make_scene(1000, 100000, 10, lm_dim=1, seed=2), hipapi.ORDER_NATURAL),
    "revisit_natural": lambda: ("revisit6000x3", scene.make_revisit_scene(6000, 120000, 3, 40, 0.3, seed=0),
                                hipapi.ORDER_NATURAL),
    "revisit_auto": lambda: ("revisit6000x3", scene.make_revisit_scene(6000, 120000, 3, 40, 0.3, seed=0),
                             hipapi.ORDER_AUTO),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default=",".join(SCENES))
    a = ap.parse_args(argv)
    for key in a.scenes.split(","):
        name, sc, mode = SCENES[key]()
        print(json.dumps(run(name, sc, mode)), flush=True)


if __name__ == "__main__":
    main()
