"""Weakest modes of the reduced system on the MI355X (ba_hip_get_weakest_modes, k_factorsolve.hip): the eigenpairs
of S of smallest magnitude by block inverse iteration on the kept factor, against numpy.linalg.eigh on the kept S.

Bounds as in test_weakest_modes.py: every eigenvalue within max(1e-9, 4.5 eps cond(S)) relative (asserted <= 1e-8
as _tol does), per pair ||numpy.linalg.solve(S, v) - v / lambda|| <= (10 tolerance + that bound) / |lambda|.  Where
numpy shows a gap |lambda_(k+1)| >= 2 |lambda_k| the subspace is compared: with R the residual block of S^-1 and
gap_theta >= theta_k / 2, sin(angle) <= ||R||_F / gap_theta <= 2 sqrt(k) (tolerance + bound) |lambda_k / lambda_1|.
The scenes that need a property of their spectrum (the gap, the scale direction) are checked for it on the CPU
with the oracle before the device is asked."""
import numpy as np
import pytest

from ba_amd import adjuster, hipapi, scene
from helpers import fill, gn_options
from oracle import pyoracle as po
from test_marginals_gpu import _engine, _solve, _sym, _tol
from test_weakest_modes import CAP, TOLERANCE, hc, host_modes, reference, subspace_sine  # noqa: F401  (hc: a fixture)

pytestmark = pytest.mark.gpu


def _check(S, lam, modes, st, tol):
    """eigenvalues, orthogonality of what came back, the per-pair numpy check; returns the reference eigenvalues"""
    k, n = len(lam), S.shape[0]
    w, _ = reference(S)
    assert st["converged"] == k and st["iterations"] < CAP, st
    ev = float(np.max(np.abs(lam - w[:k]) / np.abs(lam)))
    pair = 0.0
    for i in range(k):
        d = np.linalg.norm(np.linalg.solve(S, modes[i]) - modes[i] / lam[i])
        pair = max(pair, d * abs(lam[i]) / (10 * TOLERANCE + tol))
    orth = float(np.abs(modes @ modes.T - np.eye(k)).max())
    print("n=%d k=%d: eigenvalue err %.3g (bound %.3g), pair check %.3g of its bound, orthogonality %.3g; %s"
          % (n, k, ev, tol, pair, orth, st))
    assert ev <= tol and pair <= 1.0 and orth <= n * np.finfo(np.float64).eps
    assert np.all(np.diff(np.abs(lam)) >= 0)
    return w


def _scene(which):
    if which == 83:
        sc = scene.make_scene(83, 500, 6, lm_dim=1, seed=11)
    else:
        sc = scene.make_scene(400, 1200, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    if which == 83:
        pa[[9, 40]] = 0
    return sc, pa


@pytest.mark.parametrize("which", [83, 400])
def test_scene_modes(hc, which):  # noqa: F811
    """k = 6 on both scenes (83 poses: fixed poses and pose-pose terms): against eigh, against the host restatement on
    the same S, twice the same bits."""
    sc, pa = _scene(which)
    s = _engine(sc, 1, pa, pose_pose=which == 83)
    _solve(s)
    eng = s.eng
    S = _sym(eng.get_S())
    tol = _tol(S)
    lam, modes = eng.weakest_modes(6)
    st = eng.mode_stats()
    _check(S, lam, modes, st, tol)
    assert st["block"] == 64 and st["solve_ms"] > 0 and st["ortho_ms"] > 0 and st["workspace_bytes"] > 0
    lam2, modes2 = eng.weakest_modes(6)
    assert np.array_equal(lam, lam2) and np.array_equal(modes, modes2)
    if which == 83:   # (the restatement is plain loops: the small scene keeps the test at seconds)
        hl, _, hst = host_modes(hc, S, 6)
        print("host restatement: %s, eigenvalues differ by %.3g" % (hst, np.max(np.abs(hl - lam) / np.abs(lam))))
        assert np.max(np.abs(hl - lam) / np.abs(lam)) <= tol
    # the call leaves the other getters' state alone and the solve's statistics too
    before = eng.factor_solve_stats()
    eng.weakest_modes(2)
    assert eng.factor_solve_stats() == before
    eng.close()


def test_orderings_agree():
    sc, pa = _scene(400)
    res = []
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO):
        s = _engine(sc, 1, pa, mode=mode)
        _solve(s)
        S = _sym(s.eng.get_S())
        lam, modes = s.eng.weakest_modes(6)
        _check(S, lam, modes, s.eng.mode_stats(), _tol(S))
        res.append(lam)
        s.eng.close()
    assert np.max(np.abs(res[0] - res[1]) / np.abs(res[0])) <= _tol(S)


def _options():
    o = adjuster.default_options()
    o.use_dogleg = 0
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    o.write_reduced_camera_matrix = 1
    return o


def _with_weak_prior(P, L, k, seed, sigma):
    """One pose fixed, a unary translation prior of standard deviation sigma on the last pose: the oracle's S on the
    CPU, then the same problem solved on the device through the adjuster."""
    sc = scene.make_scene(P, L, k, lm_dim=1, seed=seed, anchors=(0,))
    act = np.ones(P, dtype=np.uint8)
    act[0] = 0
    cov = np.eye(6) * sigma ** 2
    o = po.OracleBundleAdjuster(1, 6)
    o.Init(gn_options(po))
    fill(o, sc, active=act)
    o.AddUnaryConstraint(P - 1, sc.poses[P - 1], cov, False)
    o.Solve(1)
    So = _sym(o.S())

    def device():
        h = adjuster.BundleAdjuster(1, 6)
        h.Init(_options())
        fill(h, sc, active=act)
        h.AddUnaryConstraint(P - 1, sc.poses[P - 1], cov, False)
        h.Solve(1)
        assert adjuster.RESULT_NAMES[h.summary().result] == "Success"
        return h

    return sc, act, So, device


def test_subspace_at_a_gap():
    """12 poses, k = 2: numpy's spectrum of the oracle's S has |lambda_3| >= 2 |lambda_2|, asserted before the device
    runs; the device's two modes span numpy's invariant subspace."""
    sc, act, So, device = _with_weak_prior(12, 100, 4, 21, 0.03)
    k = 2
    wo, _ = reference(So)
    assert abs(wo[k]) >= 2 * abs(wo[k - 1]), wo[:4]
    _tol(So)
    h = device()
    S = _sym(h.engine().get_S())
    tol = _tol(S)
    w, V = reference(S)
    assert abs(w[k]) >= 2 * abs(w[k - 1])
    lam, modes = h.GetWeakestModes(k)
    _check(S, lam, modes, h.GetModeStats(), tol)
    sine = subspace_sine(modes.T, V[:, :k])
    limit = 2 * np.sqrt(k) * (TOLERANCE + tol) * abs(w[k - 1] / w[0])
    print("gap %.3g at k = %d: subspace sine %.3g (limit %.3g)" % (abs(w[k] / w[k - 1]), k, sine, limit))
    assert sine <= limit


def test_full_space_n18():
    """three active poses: n = 18, the block is the whole space and the first Rayleigh-Ritz is exact"""
    sc = scene.make_scene(12, 100, 4, lm_dim=1, seed=21)
    pa = np.zeros(sc.num_poses, dtype=np.uint8)
    pa[[3, 6, 10]] = 1
    s = _engine(sc, 1, pa)
    _solve(s)
    S = _sym(s.eng.get_S())
    assert S.shape[0] == 18
    lam, modes = s.eng.weakest_modes(18)
    st = s.eng.mode_stats()
    _check(S, lam, modes, st, _tol(S))
    assert st["iterations"] == 1 and st["block"] == 18
    with pytest.raises(hipapi.HipError, match="k must be between 1 and min\\(32, n\\) = 18"):
        s.eng.weakest_modes(19)
    s.eng.close()


def test_scale_direction_is_the_weakest_mode():
    """Monocular, one pose fixed, a deliberately weak translation prior (sigma 0.0215, chosen on the CPU so that the
    preconditions below hold with the oracle's S): the weakest mode is the scale gauge (t_i - t_fixed, 0, 0, 0)."""
    sc, act, So, device = _with_weak_prior(30, 300, 6, 21, 0.0215)
    ids = np.nonzero(act)[0]
    d = np.zeros(So.shape[0])
    for a, p in enumerate(ids):
        d[6 * a:6 * a + 3] = sc.poses[p, :3] - sc.poses[0, :3]
    d /= np.linalg.norm(d)
    wo, Vo = reference(So)
    _tol(So)
    assert abs(Vo[:, 0] @ d) >= 0.99 and abs(wo[0] / wo[1]) <= 1e-2
    h = device()
    S = _sym(h.engine().get_S())
    tol = _tol(S)
    lam, modes = h.GetWeakestModes(3)
    st = h.GetModeStats()
    _check(S, lam, modes, st, tol)
    cosine = abs(modes[0] @ d)
    print("scale direction: cosine %.6f, lambda_1 / lambda_2 = %.3g" % (cosine, lam[0] / lam[1]))
    assert cosine >= 0.99
    lam_e, modes_e = h.engine().weakest_modes(3)
    assert lam_e[0] == lam[0] and np.array_equal(modes_e, modes)
    # the other layer of the adjuster: SolveWithFactor applies the inverse the mode is an eigenvector of
    X = h.SolveWithFactor(modes.T.copy())
    assert np.max(np.abs(X[:, 0] - modes[0] / lam[0])) * abs(lam[0]) <= 10 * TOLERANCE + tol
    with pytest.raises(RuntimeError, match="unavailable"):
        h.GetWeakestModes(0)
    with pytest.raises(RuntimeError, match="unavailable"):
        h.SolveWithFactor(np.zeros((S.shape[0], 513)))


def test_refusals_and_the_cap():
    sc = scene.make_scene(40, 200, 6, lm_dim=1, seed=15)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, keep=False)
    eng = s.eng
    with pytest.raises(hipapi.HipError, match="ba_hip_get_weakest_modes: needs the factor of the last ba_hip_solve_gn"):
        eng.weakest_modes(2)
    assert eng.mode_stats()["iterations"] == 0
    _solve(s)
    good = eng.weakest_modes(4)
    with pytest.raises(hipapi.HipError, match="0 modes requested, k must be between 1 and min\\(32, n\\) = 32"):
        eng.weakest_modes(0)
    with pytest.raises(hipapi.HipError, match="33 modes requested"):
        eng.weakest_modes(33)
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_weakest_modes(eng.h, 2, None, None, None))
    with pytest.raises(hipapi.HipError, match="NULL"):
        eng._chk(eng.L.ba_hip_get_mode_stats(eng.h, None))
    assert np.array_equal(eng.weakest_modes(4)[0], good[0])
    # the cap: the call succeeds, the statistics say that the pairs have not converged
    lam, modes = eng.weakest_modes(4, max_iterations=1)
    st = eng.mode_stats()
    assert st["iterations"] == 1 and st["converged"] < 4 and st["residual_max"] > TOLERANCE
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(modes))
    live = hipapi.device_bytes_live()
    eng.release_marginals()
    assert hipapi.device_bytes_live() < live
    assert np.array_equal(eng.weakest_modes(4)[1], good[1])
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="re-linearised"):
        eng.weakest_modes(2)
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=1e-8)
    assert eng.solve_gn() == 0
    with pytest.raises(hipapi.HipError, match="PCG"):
        eng.weakest_modes(2)
    eng.close()
