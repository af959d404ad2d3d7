"""Pose ordering of the reduced camera solve on the MI355X (ba_hip_set_pose_ordering): a permuted engine
computes the same S, right-hand sides, steps and states as the natural one, its public outputs are in
natural order, AUTO cuts the factor's tile products on multi-lap routes, the group graph built on the
device equals the host builder's, and sharded engines refuse an ordering."""
import numpy as np
import pytest

from ba_amd import hipapi, scene
from helpers import _add_pose_pose, rel_err

pytestmark = pytest.mark.gpu



def _engine(sc, lm_dim, pose_dim, pa, mode=hipapi.ORDER_NATURAL, perm=None, tvs=False, pose_pose=False,
            host_structure=False):
    eng = hipapi.Engine(lm_dim, pose_dim)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.keep_reduced_system = 1
    eng.set_options(o)
    if tvs:
        eng.set_calibration(0, True)
    if host_structure:
        eng.debug_set(5, 1)
    nsel = sc.obs_per_landmark + (1 if lm_dim == 1 else 0)
    keep = np.ones(len(sc.obs_pose), dtype=bool)
    if lm_dim == 1 and not hasattr(sc, "revisited"):
        keep[::nsel] = False
    if hasattr(sc, "revisited") and lm_dim == 1:
        first = np.r_[True, np.diff(sc.obs_lm) != 0]
        keep &= ~first
    eng.set_cameras(sc.cam_params, [0.01, -0.02, 0.03, 0, 0, 0, 1] if tvs else [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    if pose_pose:
        _add_pose_pose(eng, sc, sc.num_poses)
    eng.set_pose_ordering(mode)
    if perm is not None:
        eng.set_pose_permutation(perm)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    return eng


def _gn(eng, iters):
    for _ in range(iters):
        eng.linearize()
        assert eng.solve_gn() == 0
        eng.compose_step(0.0, 1.0)
        eng.apply_step()


@pytest.mark.parametrize("lm_dim,pose_dim,tvs,pose_pose", [(1, 6, False, False), (3, 6, False, True),
                                                           (1, 6, True, False), (1, 6, True, True)],
                         ids=["lm1_d6", "lm3_d6_posepose", "lm1_d6_tvs", "lm1_d6_tvs_posepose"])
def test_user_permutation_is_invisible(lm_dim, pose_dim, tvs, pose_pose):
    """A random (unaligned) permutation with inactive poses interleaved: the un-permuted S, rhs and steps
    equal the natural engine's, and iterations leave the same state."""
    sc = scene.make_scene(90, 500, 6, lm_dim=lm_dim, seed=21)
    P = sc.num_poses
    pa = np.ones(P, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    pa[[5, 33, 61]] = 0
    Pact = int(pa.sum())
    perm = np.random.default_rng(5).permutation(Pact).astype(np.uint32)
    nat = _engine(sc, lm_dim, pose_dim, pa, tvs=tvs, pose_pose=pose_pose)
    usr = _engine(sc, lm_dim, pose_dim, pa, hipapi.ORDER_USER, perm, tvs=tvs, pose_pose=pose_pose)
    got, st = usr.get_pose_ordering()
    assert np.array_equal(got, perm) and st["mode"] == hipapi.ORDER_USER
    g0, _ = nat.get_pose_ordering()
    assert np.array_equal(g0, np.arange(Pact))
    for e in (nat, usr):
        e.linearize()
        assert e.solve_gn() == 0
    Sn, Su = nat.get_S(), usr.get_S()
    assert rel_err(Su, Sn) < 1e-12
    for a, b in zip(nat.get_rhs(), usr.get_rhs()):
        assert rel_err(b, a) < 1e-10
    for a, b in zip(nat.get_delta_gn(), usr.get_delta_gn()):
        assert rel_err(b, a) < 1e-10
    for e in (nat, usr):
        e.compose_step(0.0, 1.0)
    for a, b in zip(nat.get_step(), usr.get_step()):
        assert rel_err(b, a) < 1e-10
    for e in (nat, usr):
        e.apply_step()
    _gn(nat, 2)
    _gn(usr, 2)
    # one dogleg solve on top
    for e in (nat, usr):
        e.linearize()
        assert e.solve_gn() == 0
    dn, du = nat.dogleg_terms(1), usr.dogleg_terms(1)
    for name, _ in hipapi.DoglegScalars._fields_:
        a, b = getattr(dn, name), getattr(du, name)
        assert abs(a - b) <= 1e-9 * max(abs(a), 1e-12), name
    for e in (nat, usr):
        e.compose_step(0.3, 0.5)
        e.apply_step()
        e.end_solve()
    pn, pu = nat.get_poses(P)[0], usr.get_poses(P)[0]
    assert rel_err(pu, pn) < 1e-9
    nl = sc.num_landmarks
    assert rel_err(usr.get_landmarks(nl), nat.get_landmarks(nl)) < 1e-9
    for e in (nat, usr):
        e.close()


def _revisit(P, seed=0):
    sc = scene.make_revisit_scene(P, 5 * P, laps=3, window=12, revisit_frac=0.5, seed=seed)
    pa = np.ones(P, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    return sc, pa


def _compare_auto(P, max_ratio, tol):
    sc, pa = _revisit(P)
    nat = _engine(sc, 1, 6, pa)
    aut = _engine(sc, 1, 6, pa, hipapi.ORDER_AUTO)
    perm, st = aut.get_pose_ordering()
    assert st["mode"] == hipapi.ORDER_AUTO and st["group_size"] == 32
    assert st["candidate"] != 0 and st["tile_products_chosen"] < st["tile_products_natural"]
    assert sorted(perm.tolist()) == list(range(int(pa.sum())))
    pn, pau = nat.structure_stats()["factor_tile_products"], aut.structure_stats()["factor_tile_products"]
    assert pau <= max_ratio * pn, (pau, pn)
    for e in (nat, aut):
        e.linearize()
        assert e.solve_gn() == 0
    assert rel_err(aut.get_delta_gn()[0], nat.get_delta_gn()[0]) < tol
    assert rel_err(aut.get_delta_gn()[1], nat.get_delta_gn()[1]) < tol
    for e in (nat, aut):
        e.compose_step(0.0, 1.0)
        e.apply_step()
    _gn(nat, 2)
    _gn(aut, 2)
    for e in (nat, aut):
        e.end_solve()
    assert rel_err(aut.get_poses(P)[0], nat.get_poses(P)[0]) < tol
    return nat, aut, pn, pau


def test_auto_on_a_three_lap_route_1200_poses():
    nat, aut, pn, pau = _compare_auto(1200, 0.5, 1e-8)
    nat.close()
    aut.close()


def test_auto_on_a_three_lap_route_6000_poses():
    nat, aut, pn, pau = _compare_auto(6000, 0.1, 1e-9)
    nat.close()
    aut.close()


def test_group_graph_on_device_equals_host_builder():
    sc, pa = _revisit(1200, seed=4)
    for lm_dim in (1, 3):
        dev = _engine(sc, lm_dim, 6, pa, hipapi.ORDER_AUTO, pose_pose=True)
        host = _engine(sc, lm_dim, 6, pa, hipapi.ORDER_AUTO, pose_pose=True, host_structure=True)
        gd, gh = dev.get_pose_group_graph(), host.get_pose_group_graph()
        assert len(gd[0]) == (int(pa.sum()) + 31) // 32 + 1 and len(gd[1]) > 0
        assert np.array_equal(gd[0], gh[0]) and np.array_equal(gd[1], gh[1])
        assert np.array_equal(dev.get_pose_ordering()[0], host.get_pose_ordering()[0])
        for e in (dev, host):
            e.linearize()
            assert e.solve_gn() == 0
        assert rel_err(dev.get_S(), host.get_S()) < 1e-12
        dev.close()
        host.close()


def test_sharded_engine_refuses_an_ordering():
    from ba_amd import sharding
    ar = sharding.ThreadAllReduce(2)
    eng = hipapi.Engine(1, 6)
    eng.set_allreduce(ar.hook(0), 0, 2)
    with pytest.raises(hipapi.HipError, match="sharded"):
        eng.set_pose_ordering(hipapi.ORDER_AUTO)
    eng.set_pose_ordering(hipapi.ORDER_NATURAL)
    eng.close()
    eng = hipapi.Engine(1, 6)
    eng.set_pose_ordering(hipapi.ORDER_AUTO)
    with pytest.raises(hipapi.HipError, match="natural pose order"):
        eng.set_allreduce(ar.hook(0), 0, 2)
    with pytest.raises(hipapi.HipError, match="natural pose order"):
        eng.set_collectives(lambda op, ptr, count, root: 0)
    eng.close()


def test_cpp_options_pose_ordering_auto_gives_the_same_result():
    """include/ba/BundleAdjuster.h with Options::pose_ordering = Auto (visual_ba_demo --ordering auto): the
    same errors as the default run, and the ordering statistics of the engine printed."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ba_amd", "lib", "visual_ba_demo")
    runs = [subprocess.run([exe] + extra, capture_output=True, text=True, timeout=120)
            for extra in ([], ["--ordering", "auto"])]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
    assert "pose ordering: mode 1" in runs[1].stdout
    line = [[ln for ln in r.stdout.splitlines() if ln.startswith("proj error")][0] for r in runs]
    assert line[0] == line[1]
