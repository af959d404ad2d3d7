"""The bulk LDL^T update launched from its lists of non-empty blocks (bulk_lists.h) against the grid launch over the
whole block triangle (BA_HIP_BULK_GRID=1), on the MI355X.

Both launches run the same blocks, one workgroup per 128-block per launch, with the same K order, so every result
must agree bit for bit: there is no tolerance.  BA_HIP_KOUT = 16 and BA_HIP_BULK_FULL_M = 16 as in
test_bulk_update_epilogue_gpu.py, so the 128-block launches run at 48 - 96 tiles.

(i)  The stand-alone solve (ba_hip_tile_solve: a list built for the call's own pattern and dropped after it) on
     every small pattern of test_bulk_block_lists.py: the seven schedule cases, dense96, noblock48 (a launch whose
     list is empty) and oneblock48 (one block and seven sentinels).  x, the pattern, the factor storage, linvT and
     dsgn are bitwise equal between two identical calls and between the two launches, and the backward-error
     ratios of tile_factor_cases.check_factor are below 1 (the CPU file shows that a float64 reference meets them).
(ii) The engine's cached lists: one engine on a scene of 520 poses (49 tile columns, a circular band), two
     Gauss-Newton solves with a step between them (the second reuses the lists), then the same problem under another
     pose ordering (the pattern version moves, the lists are rebuilt) and a third solve.  The Gauss-Newton steps of
     all three solves are bitwise equal to those of the same sequence under BA_HIP_BULK_GRID=1.

BA_HIP_BULK_LISTS_REPORT=1 makes the library print one line per build of the lists: the children's lines show that
the list path ran (built 1), that the second solve of (ii) built nothing and that the new ordering built again.

Every case runs two child processes (the switch is read once per process), each with its own time limit; a child
that ends on a signal or at its limit fails the test and is not run again.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import test_bulk_block_lists as bl  # noqa: E402
import tile_factor_cases as tf  # noqa: E402

ARRAYS = ("x", "nzL", "storage", "linvT", "dsgn")
SCENE_POSES, SCENE_LANDMARKS = 520, 6000
STEPS = ("first", "cached", "reordered")
SWITCHES = ("BA_HIP_LEFT_MIN_TILES", "BA_HIP_SQUARE", "BA_HIP_SQ_W", "BA_HIP_NO128", "BA_HIP_NO_LOOKAHEAD",
            "BA_HIP_BULK_FULL", "BA_HIP_C_RMW", "BA_HIP_BULK_GRID", "BA_HIP_DENSE", "BA_HIP_NO_DIST_SOLVE")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_tile_case(name, check):
    """Child process: the device factor of one pattern, twice; prints a digest per array."""
    from ba_amd import hipapi
    c = bl.build(name)
    a = tf.lower_dense(c)
    eng = hipapi.Engine(1, 6)
    try:
        outs = []
        for _ in range(2):
            x, rc, nzL, st, linvT, dsgn = eng.tile_solve(a, c.b, c.tile_map, keep_factor=True)
            assert rc == 0, c.name
            outs.append((x, nzL, st, linvT, dsgn))
        for what, p, q in zip(ARRAYS, outs[0], outs[1]):
            assert p.tobytes() == q.tobytes(), "%s: %s differs between two identical calls" % (c.name, what)
        rf, rs = tf.check_factor(c, *outs[0]) if check else (0.0, 0.0)
    finally:
        eng.close()
    for what, p in zip(ARRAYS, outs[0]):
        print("DIGEST %s %s" % (what, digest(p)))
    if check:
        print("RATIO %s: factor %.3g solve %.3g" % (name, rf, rs))
    assert rf < 1.0 and rs < 1.0
    print("CASE-OK " + name)


def run_engine_case():
    """Child process: three Gauss-Newton solves of one engine; prints a digest of each step."""
    from ba_amd import hipapi, scene
    sc = scene.make_scene(SCENE_POSES, SCENE_LANDMARKS, 10, lm_dim=1, seed=5)
    pa = np.ones(SCENE_POSES, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    keep[::sc.obs_per_landmark + 1] = False          # the reference observations
    eng = hipapi.Engine(1, 6)

    def upload(mode, perm=None):
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
        eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
        eng.set_pose_ordering(mode)
        if perm is not None:
            eng.set_pose_permutation(perm)
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(SCENE_POSES, dtype=np.uint16))

    def solve(step):
        eng.linearize()
        assert eng.solve_gn() == 0, step
        for k, d in enumerate(eng.get_delta_gn()):
            assert np.all(np.isfinite(d)), step
            print("DIGEST %s.%d %s" % (step, k, digest(d)))

    try:
        upload(hipapi.ORDER_NATURAL)
        nt = (eng.num_pose_params() + 63) // 64
        assert nt >= 48, nt
        print("TILES %d" % nt)
        solve("first")
        eng.compose_step(0.0, 1.0)
        eng.apply_step()
        solve("cached")
        nact = eng.num_pose_params() // 6
        perm = np.r_[np.arange(0, nact, 2), np.arange(1, nact, 2)].argsort().astype(np.uint32)   # even poses first
        upload(hipapi.ORDER_USER, perm)
        solve("reordered")
    finally:
        eng.close()
    print("CASE-OK engine")


def children(args, name):
    """The two children of one case; {mode: {what: digest}}."""
    base = dict(os.environ, BA_HIP_BULK_FULL_M="16", BA_HIP_KOUT="16", BA_HIP_BULK_LISTS_REPORT="1")
    for k in SWITCHES:
        base.pop(k, None)
    digests = {}
    for mode in ("lists", "grid"):
        env = dict(base, BA_HIP_BULK_GRID="1") if mode == "grid" else base
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args + [mode], env=env, capture_output=True,
                           text=True, timeout=180)
        print("\n".join(mode + " " + l for l in r.stdout.splitlines() if l.startswith(("RATIO", "TILES"))))
        assert r.returncode == 0, mode + ": " + r.stdout[-3000:] + r.stderr[-3000:]
        assert "CASE-OK " + name in r.stdout, mode + ": " + r.stdout[-2000:]
        digests[mode] = dict(l.split()[1:3] for l in r.stdout.splitlines() if l.startswith("DIGEST"))
        # "bulk lists: nblk N kout K built B launches L blocks M ...": (built, launches, blocks) per build
        digests[mode]["builds"] = [tuple(int(l.split()[k]) for k in (7, 9, 11)) for l in r.stderr.splitlines()
                                   if l.startswith("bulk lists:")]
    return digests


@pytest.mark.gpu
@pytest.mark.parametrize("name", bl.SMALL)
def test_standalone_solve_agrees_with_the_grid_launch(name):
    d = children(["tile", name], name)
    builds = {mode: d[mode].pop("builds") for mode in d}
    assert len(builds["lists"]) == 2 and len(builds["grid"]) == 2          # one per call: the list is the call's own
    assert all(b[:2] == (1, 1 if name != "dense96" else 4) for b in builds["lists"])
    assert all(b == (0, 0, 0) for b in builds["grid"])
    assert sorted(d["lists"]) == sorted(ARRAYS) and sorted(d["grid"]) == sorted(ARRAYS)
    for what in ARRAYS:
        assert d["lists"][what] == d["grid"][what], "%s: %s differs between the list and the grid launch" % (name, what)


@pytest.mark.gpu
def test_cached_lists_agree_with_the_grid_launch():
    d = children(["engine"], "engine")
    builds = {mode: d[mode].pop("builds") for mode in d}
    assert len(builds["lists"]) == 2, builds                                # first solve and new ordering; not the second solve
    assert all(b[:2] == (1, 1) and b[2] > 0 for b in builds["lists"]), builds
    assert all(b == (0, 0, 0) for b in builds["grid"])
    want = sorted("%s.%d" % (s, k) for s in STEPS for k in range(2))
    assert sorted(d["lists"]) == want and sorted(d["grid"]) == want
    assert len({d["lists"]["%s.0" % s] for s in STEPS}) == 3        # three different systems were solved
    for what in want:
        assert d["lists"][what] == d["grid"][what], "%s differs between the list and the grid launch" % what


if __name__ == "__main__":
    if sys.argv[1] == "tile":
        run_tile_case(sys.argv[2], sys.argv[3] == "lists")
    else:
        run_engine_case()
