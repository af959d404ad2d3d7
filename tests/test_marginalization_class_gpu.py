"""Marginalize / AddDensePrior through the C++ class (ba::BundleAdjuster via the flat C wrapper and
ba_amd/adjuster.py) on a visual-inertial window: Solve; Marginalize; Solve equals Solve; Solve bit for bit, and
Gauss-Newton and dogleg with a carried prior converge to the same state."""
import numpy as np
import pytest

from ba_amd import adjuster, scene

pytestmark = pytest.mark.gpu

P = 30


def _scene():
    sc = scene.make_scene(P, 300, 6, lm_dim=1, seed=3, outlier_frac=0.0)
    scene.add_inertial(sc, period=60.0 * P / 100.0, seed=3)
    return sc


def _window(sc, dog=0, tight=False):
    b = adjuster.BundleAdjuster(1, 15)
    o = adjuster.default_options()
    o.use_dogleg = dog
    if tight:
        o.error_change_threshold = 0.0
        o.param_change_threshold = 1e-13
    b.Init(o)
    scene.populate(b, sc, imu=True, priors=True, unary_every=10)
    return b


def _lms(sc, M):
    M = set(M)
    L = set(int(l) for p, l in zip(sc.obs_pose, sc.obs_lm) if int(p) in M)
    L |= set(int(l) for l in range(sc.num_landmarks) if int(sc.lm_ref_pose[l]) in M)
    return sorted(L)


def test_marginalize_leaves_later_solves_bitwise():
    sc = _scene()
    a, b = _window(sc), _window(sc)
    a.Solve(3)
    b.Solve(3)
    m = a.Marginalize([1], _lms(sc, [1]))
    assert len(m["pose_ids"]) > 0 and np.array_equal(m["H"], m["H"].T)
    a.Solve(3)
    b.Solve(3)
    for x, y in zip(a.poses(), b.poses()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.landmarks(), b.landmarks())


def test_gauss_newton_and_dogleg_agree_with_a_prior():
    sc = _scene()
    src = _window(sc)
    src.Solve(3)
    m = src.Marginalize([1], _lms(sc, [1]))
    out = []
    for dog in (0, 1):
        w = _window(sc, dog=dog, tight=True)
        assert w.AddDensePrior(m["pose_ids"], m) == 0
        w.Solve(60)
        out.append(w.poses()[0])
    d = np.abs(out[0] - out[1]).max()
    assert d <= 1e-8, d


def test_class_refusals():
    sc = _scene()
    a = _window(sc)
    with pytest.raises(RuntimeError):
        a.Marginalize([1], _lms(sc, [1]))  # no Solve() yet
    a.Solve(1)
    with pytest.raises(RuntimeError):
        a.Marginalize([], [])
    bad = {"pose_ids": np.array([1, 2], np.uint32), "x0": np.zeros((1, 16)), "H": np.eye(15), "b": np.zeros(15), "c": 0.0}
    with pytest.raises(RuntimeError):
        a.AddDensePrior([1, 2], bad)  # sizes do not match
