"""Ownership of device memory on the MI355X: every buffer belongs to its engine (or to the call that made it) and is
freed with it.  Measured with ba_hip_device_bytes_live, the byte count of the engine's own buffers over all engines
of the process, so nothing another tenant of the card does moves it.  All scenes are make_scene(12, 60, 4) with the
first two poses fixed; all stand-alone systems have n = 65: two tiles, a padded diagonal, the right-hand-side row
behind the padding."""
import gc
import threading

import numpy as np
import pytest

from ba_amd import hipapi, scene, sharding
import leverage_cases as lc

pytestmark = pytest.mark.gpu

live = hipapi.device_bytes_live
N = 65


def _scene(lm_dim):
    sc = scene.make_scene(12, 60, 4, lm_dim=lm_dim, seed=11)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[:2] = 0
    return sc, pa


def _system(seed=5):
    """(A, b): symmetric positive definite, n = 65, every tile nonzero"""
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(N, N))
    return m @ m.T + N * np.eye(N), rng.normal(size=N)


def _landmarks_of(s, pose):
    """every landmark observed from `pose` or (LmSize 1) anchored in it: what marginalising the pose takes along"""
    lms = set(int(l) for p, l in zip(s.obs_pose, s.obs_lm) if int(p) == pose)
    if s.lm_dim == 1:
        lms |= set(int(l) for l in range(s.sc.num_landmarks) if int(s.sc.lm_ref_pose[l]) == pose)
    return sorted(lms)


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_everything_comes_back(lm_dim):
    """One engine through every feature that allocates: the count rises on the way and is back at its start, to
    the byte, after close()."""
    base = live()
    sc, pa = _scene(lm_dim)
    s = lc.engine(sc, lm_dim, pa, pose_pose=True)   # keep_reduced_system on; finalize, begin_solve
    eng = s.eng
    act = [int(p) for p in np.nonzero(pa)[0]]
    lc.solve(s)
    after_solve = live()
    assert after_solve > base
    eng.compute_marginals()
    eng.pose_marginals(act)
    eng.landmark_marginals()
    eng.joint_marginals([act[0], act[3], act[6]])
    eng.projection_leverages()
    assert live() > after_solve
    eng.marginalize([5], _landmarks_of(s, 5))
    eng.set_reduced_solver(hipapi.SOLVER_PCG, coarse_aggregate=2)
    lc.solve(s)
    A, b = _system()
    assert eng.dense_solve(A, b)[1] == 0
    assert eng.pcg_solve(A, b, 6, 1e-10)[1] == 0
    assert eng.tile_solve(A, b)[1] == 0
    assert eng.select_kth(np.abs(b), 7) == np.sort(np.abs(b))[7]   # (the selection is over non-negative errors)
    top = live()
    print("lm%d: base %d, after the first solve %d, at the end %d bytes" % (lm_dim, base, after_solve, top))
    eng.close()
    assert live() == base


def test_the_class_too():
    """PoseSize 15 with inertial residuals through ba::BundleAdjuster (adjuster.py -> ba_capi): deleting the object
    gives everything back."""
    from ba_amd import adjuster
    base = live()
    P = 12
    sc = scene.make_scene(P, 60, 4, lm_dim=1, seed=2)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    o = adjuster.default_options()
    o.use_dogleg = 1
    o.write_reduced_camera_matrix = 1
    h = adjuster.BundleAdjuster(1, 15)
    h.Init(o)
    pa = np.ones(P, dtype=np.uint8)
    pa[:2] = 0
    scene.populate(h, sc, active=pa, imu=True, priors=True, unary_every=3)
    h.Solve(1)
    assert adjuster.RESULT_NAMES[h.summary().result] not in ("FactorizationError", "SolverError")
    assert live() > base
    del h
    gc.collect()
    assert live() == base


def test_stand_alone_solves_keep_nothing_of_their_own():
    """The same system twice through each stand-alone solve: the first call may grow work space the engine owns,
    the second leaves the count where it was, and x is bitwise the same."""
    base = live()
    eng = hipapi.Engine(1, 6)
    A, b = _system()
    for name, call in (("dense_solve", lambda: eng.dense_solve(A, b)),
                       ("pcg_solve", lambda: eng.pcg_solve(A, b, 6, 1e-10, coarse_aggregate=2)),
                       ("tile_solve", lambda: eng.tile_solve(A, b, np.tril(np.ones((2, 2), dtype=np.uint8))))):
        r1 = call()
        c1 = live()
        r2 = call()
        c2 = live()
        print("%s: %d bytes after the first call, %d after the second" % (name, c1, c2))
        assert r1[1] == 0 and r2[1] == 0
        assert c1 == c2, name
        assert np.array_equal(r1[0], r2[0]), name
        assert np.abs(A @ r1[0] - b).max() <= 1e-8 * np.abs(b).max(), name   # (cond(A) < 10; PCG stops at 1e-10)
    eng.close()
    assert live() == base


def test_refusals_allocate_nothing():
    """Four refused calls: today's message, and the count does not move across any of them."""
    sc, pa = _scene(1)
    s = lc.engine(sc, 1, pa)
    eng = s.eng
    A, b = _system()

    def refused(match, call):
        before = live()
        with pytest.raises(hipapi.HipError, match=match):
            call()
        assert live() == before, match

    refused("ba_hip_get_pose_marginals: needs the factor of the last ba_hip_solve_gn", lambda: eng.pose_marginals([2]))
    refused("ba_hip_pcg_solve: block must lie in 1 .. 16", lambda: eng.pcg_solve(A, b, 17, 1e-8))
    assert A[64, 0] != 0.0
    refused(r"ba_hip_tile_solve: entry \(64, 0\) is nonzero but tile \(1, 0\) is not in the tile map",
            lambda: eng.tile_solve(A, b, np.eye(2, dtype=np.uint8)))
    lc.solve(s)
    many = np.arange(hipapi.JOINT_MAX_COLUMNS // 6 + 1) % sc.num_poses   # the column count is checked before the ids
    refused("%d columns requested, the limit is BA_HIP_JOINT_MAX_COLUMNS" % (6 * len(many)),
            lambda: eng.joint_marginals(many))
    eng.close()


def test_the_promised_releases_still_release():
    """release_marginals gives back at least the store while the engine lives; the next request recomputes the
    same bits."""
    base = live()
    sc, pa = _scene(1)
    s = lc.engine(sc, 1, pa, pose_pose=True)
    eng = s.eng
    act = [int(p) for p in np.nonzero(pa)[0]]
    lc.solve(s)
    eng.compute_marginals()
    first = eng.pose_marginals(act)
    store = eng.marginal_stats()["store_bytes"]
    assert store > 0
    before = live()
    eng.release_marginals()
    print("release_marginals: %d -> %d bytes, store %d" % (before, live(), store))
    assert before - live() >= store
    assert np.array_equal(eng.pose_marginals(act), first)
    eng.close()
    assert live() == base


def test_a_sharded_engine():
    """Two ranks in one process (thread-emulated all-reduce), half of the landmarks each: one linearize + solve_gn,
    both engines closed, everything back."""
    base = live()
    sc, pa = _scene(1)
    sel = np.ones(len(sc.obs_pose), dtype=bool)
    sel[::sc.obs_per_landmark + 1] = False   # LmSize 1: the reference pose's own observation is no residual
    z, pose, lm = sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel]
    engs = []
    for ids in (np.arange(0, 30), np.arange(30, 60)):
        new_id = np.full(sc.num_landmarks, -1, dtype=np.int64)
        new_id[ids] = np.arange(len(ids))
        mine = new_id[lm] >= 0
        eng = hipapi.Engine(1, 6)
        eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
        eng.set_poses(sc.poses, is_active=pa)
        eng.set_landmarks(sc.landmarks[ids], sc.lm_ref_pose[ids])
        eng.set_projection_residuals(z[mine], pose[mine], new_id[lm[mine]].astype(np.uint32))
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
        engs.append(eng)
    ar = sharding.ThreadAllReduce(2)
    out = {}

    def run(r):
        try:
            engs[r].linearize()
            out[r] = engs[r].solve_gn()
        except Exception as exc:   # reported by the assertion below
            out[r] = exc
            ar.barrier.abort()

    for r in range(2):
        engs[r].set_allreduce(ar.hook(r), r, 2)
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not ar.failed and out == {0: 0, 1: 0}, out
    assert live() > base
    for eng in engs:
        eng.close()
    assert live() == base
