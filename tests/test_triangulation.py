"""Landmark triangulation with the poses held fixed, on the CPU: the rules of ba_amd/csrc/triang.h through the host
restatement ba_hostcheck_triangulate (the functions the kernel of k_triang.hip applies), against ground truth, against
hand-built landmarks for every status, and against the numpy restatement of tests/triangulation_cases.py."""
import numpy as np
import pytest

import triangulation_cases as tc
from ba_amd import scene
from helpers import hostcheck_lib

EPS = tc.EPS


@pytest.fixture(scope="module")
def hc():
    return hostcheck_lib()


# ---- closed forms on noise-free scenes against ground truth ------------------------------------------------------------
EXACT = [(16, 60, 4, 2), (24, 200, 2, 3), (66, 120, 3, 1)]


def _midpoint_condition(c, l):
    """cond2 of A = sum (I - d d^T) over the bearings of landmark l: the conditioning of the intersection of its rays.
    LmSize 1 solves for the depth along the reference ray only, but the point it returns is the intersection of the same
    bundle — the reference ray and the observations — so the reference ray joins the sum."""
    tws, tsw = tc.tables(c)
    A = np.zeros((3, 3))
    cam = lambda a: tuple(c.cam_params[c.cam[a]]) + (c.cam_w[c.cam[a]], int(c.cam_model[c.cam[a]]))
    for a in np.nonzero(c.lm == l)[0]:
        d = tsw[c.pose[a]][c.cam[a]][0].T @ tc.bearing(cam(a), c.z[a])
        A += np.eye(3) - np.outer(d, d)
    if c.lm_dim == 1:
        d = c.x_w[l, :3] / np.linalg.norm(c.x_w[l, :3])     # (directions_only: x_w is the world bearing of the reference ray)
        A += np.eye(3) - np.outer(d, d)
    return np.linalg.cond(A)


@pytest.mark.parametrize("lm_dim", (1, 3))
@pytest.mark.parametrize("P,L,k,seed", EXACT)
def test_closed_form_meets_ground_truth(hc, P, L, k, seed, lm_dim):
    """True pixels, true poses, landmarks uploaded as directions only (LmSize 1) or at a wrong range (LmSize 3): the linear
    estimate alone (max_iterations = 0) is the ground-truth point to 8 cond2(A) eps relative, the REDUCED_BOUND form of
    test_damping.py.  Checked in numpy when the test was written: the midpoint meets ground truth to <= 1.9e-12
    relative, cond2(A) <= 5.3e4, smallest parallax 8.7e-3 rad."""
    sc = tc.exact_scene(P, L, k, lm_dim, seed)
    c = tc.directions_only(tc.case_from_scene(sc, lm_dim))
    res, xw, _ = tc.triangulate_host(hc, c, dict(max_iterations=0))
    assert set(res[:, 0]) <= {tc.OK, tc.NOT_CONVERGED}      # (both are written: the linear estimate is the result)
    assert np.all(res[:, 1] == k) and np.all(res[:, 2] == 0)
    pts = xw[:, :3] / xw[:, 3:4]
    gt = sc.gt_landmarks[:, :3]
    worst = 0.0
    for l in range(L):
        cond = _midpoint_condition(c, l)
        assert cond <= 5.3e4
        err = np.linalg.norm(pts[l] - gt[l]) / np.linalg.norm(gt[l])
        worst = max(worst, err / (8.0 * cond * EPS))
        assert err <= 8.0 * cond * EPS, (l, err, cond)
    assert res[:, 5].min() >= 8.7e-3
    print("closed form, P %d LmSize %d: worst error / bound %.3g, smallest parallax %.3g" % (P, lm_dim, worst, res[:, 5].min()))
    # the numpy restatement agrees on the same input
    nres, nxw, _ = tc.triangulate_numpy(c, dict(max_iterations=0))
    npts = nxw[:, :3] / nxw[:, 3:4]
    for l in range(L):
        assert np.linalg.norm(npts[l] - gt[l]) <= 8.0 * _midpoint_condition(c, l) * EPS * np.linalg.norm(gt[l])


# ---- status rules, one hand-built landmark each ----------------------------------------------------------------------
CAM = np.array([500.0, 500.0, 320.0, 240.0])
IDENT = [0.0, 0.0, 0.0, 1.0]


def _pix(pose, X):
    p = scene.quat_to_rot(np.asarray(pose[3:7])).T @ (np.asarray(X) - np.asarray(pose[:3]))
    return np.array([CAM[0] * p[0] / p[2] + CAM[2], CAM[1] * p[1] / p[2] + CAM[3]])


def _hand(lm_dim, poses, X, obs_poses, z=None, x_w=None):
    """one landmark at X seen from obs_poses (pixels z, default near the true ones), reference pose 0"""
    c = tc.Case()
    c.lm_dim = lm_dim
    c.poses = np.array(poses, dtype=np.float64)
    c.cam_params, c.cam_tvs = CAM.reshape(1, 4).copy(), np.array([[0.0, 0, 0, 0, 0, 0, 1]])
    c.cam_model, c.cam_w, c.pose_cam, c.lm_active = np.zeros(1, dtype=np.int32), np.zeros(1), None, None
    c.x_w = np.array([list(X) + [1.0] if x_w is None else x_w], dtype=np.float64)
    c.ref_pose, c.ref_cam = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    c.pose = np.array(obs_poses, dtype=np.uint32)
    # (a third of a pixel off the true ones, alternating: with exact pixels E is rounding noise and so is every stop rule)
    true = [_pix(poses[p], X) + (0.3 if i % 2 else -0.3) * np.array([1.0, -0.5]) for i, p in enumerate(obs_poses)]
    c.z = np.array(true if z is None else z, dtype=np.float64).reshape(-1, 2)
    c.lm, c.cam, c.weight = np.zeros(len(c.pose), dtype=np.uint32), np.zeros(len(c.pose), dtype=np.uint32), np.ones(len(c.pose))
    return c


POSES = [[0.0, 0, 0] + IDENT, [1.0, 0, 0] + IDENT, [0.0, 1.0, 0] + IDENT, [1.0, 0, 0] + IDENT, [0.5, 0, 3.0] + IDENT,
         [-0.5, 0.2, 3.0] + IDENT]
X0 = [0.3, -0.2, 6.0]


def _both(hc, c, opts=None):
    """status of the single landmark from the host restatement, checked against numpy's"""
    res, xw, _ = tc.triangulate_host(hc, c, opts)
    nres, _, _ = tc.triangulate_numpy(c, opts)
    assert res[0, 0] == nres[0, 0], (tc.NAMES[int(res[0, 0])], tc.NAMES[int(nres[0, 0])])
    return int(res[0, 0]), res[0], xw[0]


@pytest.mark.parametrize("lm_dim", (1, 3))
def test_status_rules(hc, lm_dim):
    held = np.array(X0 + [1.0])
    unchanged = lambda xw: np.array_equal(xw.view(np.uint64), held.view(np.uint64))
    # 0 and 1 observations
    for obs in ([], [1]):
        st, r, xw = _both(hc, _hand(lm_dim, POSES, X0, obs))
        assert st == tc.TOO_FEW_VIEWS and r[1] == len(obs) and unchanged(xw)
    # two observations from one position (poses 1 and 3 coincide; LmSize 1: both at the reference sensor)
    same = [1, 3] if lm_dim == 3 else [0, 0]
    pp = POSES if lm_dim == 3 else [POSES[0], POSES[1]]
    st, r, xw = _both(hc, _hand(lm_dim, pp, X0, same))
    assert st == tc.TOO_FEW_VIEWS and r[1] == 2 and unchanged(xw)
    # a good landmark: OK, and the point is X0
    st, r, xw = _both(hc, _hand(lm_dim, POSES, X0, [1, 2]))
    assert st == tc.OK and np.allclose(xw[:3] / xw[3], X0, rtol=0, atol=0.05)
    # parallax just under and just over min_parallax
    par = r[5]
    assert 0.1 < par < 0.3
    st, r, xw = _both(hc, _hand(lm_dim, POSES, X0, [1, 2]), dict(min_parallax=par * (1 + 1e-9)))
    assert st == tc.LOW_PARALLAX and unchanged(xw)
    st, r, xw = _both(hc, _hand(lm_dim, POSES, X0, [1, 2]), dict(min_parallax=par * (1 - 1e-9)))
    assert st == tc.OK
    # pixels that agree on a point of the reference ray at depth 2, behind the two observing sensors at z = 3 (a
    # projection does not see the sign): the linear estimate puts it there
    Xb = np.array(X0) / X0[2] * 2.0
    c = _hand(lm_dim, POSES, X0, [4, 5], z=[_pix(POSES[4], Xb), _pix(POSES[5], Xb) + [0.2, 0.1]])
    st, r, xw = _both(hc, c)
    assert st == tc.BEHIND_CAMERA and r[6] <= 0 and unchanged(xw)
    # a NaN pixel
    c = _hand(lm_dim, POSES, X0, [1, 2])
    c.z[1, 0] = np.nan
    st, r, xw = _both(hc, c)
    assert st == tc.FAILED and unchanged(xw)


def test_request_checks(hc):
    sc = tc.exact_scene(16, 60, 4, 3, 2)
    c = tc.case_from_scene(sc, 3)
    L = len(c.x_w)
    assert "is named twice" in tc.triangulate_host(hc, c, ids=[3, 7, 3])
    assert "id %d is not a landmark" % L in tc.triangulate_host(hc, c, ids=[0, L])
    assert "max_iterations 65" in tc.triangulate_host(hc, c, dict(max_iterations=65))
    assert "must not be negative" in tc.triangulate_host(hc, c, dict(step_tolerance=-1e-9))
    assert "must not be negative" in tc.triangulate_host(hc, c, dict(gradient_tolerance=-1.0))
    res, _, _ = tc.triangulate_host(hc, c, dict(max_iterations=64), ids=[5, 2])
    assert sorted(np.nonzero(res[:, 0] >= 0)[0]) == [2, 5]


# ---- host restatement against the numpy restatement on noisy scenes ------------------------------------------------------
NOISY = [(16, 60, 4, 2, 0.02), (66, 120, 3, 1, 0.0), (66, 120, 3, 1, 0.02)]
# The bound's first term, 2 step_tolerance |x|, is the distance two runs can have that both stopped on an accepted step
# of at most step_tolerance (|x| + step_tolerance); its second, 8 cond2(V + lambda D) eps |x|, the rounding of the last
# solve.  gradient_tolerance stays at its default: asked for less than about sqrt(eps) the cost-decrease test cannot
# rank the steps any more and a run stalls until the iteration limit.  step_tolerance 1e-9 is tight
# enough for the stop to come with a small last step and large enough that the first term dominates the second
# (cond2 <= 3e5 here: 8 cond2 eps <= 6e-10).
STEP_TOL = 1e-9


@pytest.mark.parametrize("lm_dim", (1, 3))
@pytest.mark.parametrize("P,L,k,seed,outliers", NOISY)
def test_host_restatement_matches_numpy(hc, P, L, k, seed, outliers, lm_dim):
    sc = scene.make_scene(P, L, k, lm_dim=lm_dim, seed=seed, outlier_frac=outliers)
    c = tc.case_from_scene(sc, lm_dim)
    o = dict(step_tolerance=STEP_TOL, max_iterations=64)
    res, xw, _ = tc.triangulate_host(hc, c, o)
    nres, nxw, fin = tc.triangulate_numpy(c, o)
    assert np.array_equal(res[:, 0], nres[:, 0]), np.nonzero(res[:, 0] != nres[:, 0])[0]
    assert np.array_equal(res[:, 1], nres[:, 1])
    worst = 0.0
    for l in range(L):
        if res[l, 0] == tc.OK:      # (a run that the iteration limit ended took no final step: the bound's first term has no footing)
            bound = tc.coordinate_bound(c, fin, l, STEP_TOL)
            err = np.linalg.norm(tc.params(c, xw)[l] - tc.params(c, nxw)[l])
            worst = max(worst, err / bound)
            assert err <= bound, (l, err, bound, res[l], nres[l])
        elif res[l, 0] != tc.NOT_CONVERGED:
            assert np.array_equal(xw[l].view(np.uint64), c.x_w[l].view(np.uint64))      # bit for bit as they were
    print("host against numpy, P %d LmSize %d outliers %g: worst |dx| / bound %.3g; iteration counts differ on %d landmarks"
          % (P, lm_dim, outliers, worst, int(np.sum(res[:, 2] != nres[:, 2]))))
    assert np.allclose(res[:, 3:6], nres[:, 3:6], rtol=1e-6, atol=1e-9, equal_nan=True)
