"""Weakest modes of S from its factor (ba_amd/csrc/factorsolve.h: block inverse iteration with Rayleigh-Ritz on
64 vectors), checked on the CPU through libba_hostcheck.so against numpy.linalg.eigh.

Bounds (eps = 2^-52, tolerance = the solver's 1e-8):
    eigenvalue   |lambda_i - ref_i| <= max(1e-9, 4.5 eps cond(S)) |lambda_i|: a backward error c eps ||S|| in applying
                 S^-1 moves lambda_i by at most c eps cond(S) |lambda_min|; the Ritz error is quadratic in the 1e-8
                 residual and negligible
    orthogonal   ||V V^T - I||_max <= n eps over the k returned modes
    per pair     ||numpy.linalg.solve(S, v) - v / lambda||_2 <= (10 tolerance + forward bound) / |lambda|: the solver's
                 own stopping criterion re-evaluated with numpy's solve
    iterations   below the cap
The matrices keep the eigenvalue bound at or below 1e-8 with two exceptions the cases themselves force: the graded
matrix (eigenvalues 10^(j/20), j < 200, so cond(S) = 10^9.95 and the bound is 8.9e-6) and the near-singular one
(cond = 1e9 by construction), where only lambda_1 / lambda_2 and the vector are checked."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)
EPS = np.finfo(np.float64).eps
TOLERANCE, CAP = 1e-8, 50


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_weakest_modes.restype = ctypes.c_int
    return lib


def host_modes(hc, S, k, tolerance=TOLERANCE, max_iterations=CAP, seed=1, pad_nonzero=False):
    """(eigenvalues (k), modes (k, n), stats dict) of the host restatement"""
    n = S.shape[0]
    S = np.ascontiguousarray(S, dtype=np.float64)
    lam, modes = np.zeros(k), np.zeros((k, n))
    out = np.zeros(3, dtype=np.uint32)
    res = ctypes.c_double()
    rc = hc.ba_hostcheck_weakest_modes(n, S.ctypes.data_as(dp), None, k, ctypes.c_double(tolerance), max_iterations, seed,
                                       int(pad_nonzero), lam.ctypes.data_as(dp), modes.ctypes.data_as(dp),
                                       out.ctypes.data_as(u32p), ctypes.byref(res))
    assert rc == 0
    return lam, modes, {"iterations": int(out[0]), "converged": int(out[1]), "block": int(out[2]), "residual_max": res.value}


def with_spectrum(ev, seed):
    """symmetric matrix with the eigenvalues `ev` and a random orthogonal eigenbasis"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((len(ev), len(ev))))[0]
    S = (Q * np.asarray(ev)) @ Q.T
    return 0.5 * (S + S.T)


def reference(S):
    """numpy's eigenpairs ordered by ascending magnitude"""
    w, V = np.linalg.eigh(S)
    o = np.argsort(np.abs(w), kind="stable")
    return w[o], V[:, o]


def bound(S, limit=1e-8):
    w = np.abs(np.linalg.eigvalsh(S))
    tol = max(1e-9, 4.5 * EPS * w.max() / w.min())
    assert limit is None or tol <= limit, "matrix too ill-conditioned for the check: %g" % tol
    return tol


def check_pairs(S, lam, modes, st, tol, eigenvalues=True):
    """the checks of the module docstring; returns the figures"""
    n, k = S.shape[0], len(lam)
    w, _ = reference(S)
    assert st["converged"] == k and st["iterations"] < CAP, st
    ev_err = float(np.max(np.abs(lam - w[:k]) / np.abs(lam)))
    orth = float(np.abs(modes @ modes.T - np.eye(k)).max())
    pair = 0.0
    for i in range(k):
        d = np.linalg.norm(np.linalg.solve(S, modes[i]) - modes[i] / lam[i])
        pair = max(pair, d * abs(lam[i]) / (10 * TOLERANCE + tol))
    print("n=%d k=%d: eigenvalue err %.3g (bound %.3g), orthogonality %.3g (n eps %.3g), pair check %.3g of its bound; %s"
          % (n, k, ev_err, tol, orth, n * EPS, pair, st))
    if eigenvalues:
        assert ev_err <= tol
    assert orth <= n * EPS
    assert pair <= 1.0
    return ev_err, orth, pair


def subspace_sine(A, B):
    """largest principal-angle sine between the column spaces of A and B (orthonormal columns)"""
    s = np.linalg.svd(A.T @ B, compute_uv=False)
    return float(np.sqrt(max(0.0, 1.0 - s.min() ** 2)))


def test_graded_spd(hc):
    S = with_spectrum(10.0 ** (np.arange(200) / 20.0), 1)
    tol = bound(S, None)   # 8.9e-6: the case fixes cond(S) at 10^9.95 (module docstring)
    for k in (1, 6, 16):
        lam, modes, st = host_modes(hc, S, k)
        check_pairs(S, lam, modes, st, tol)
        assert st["block"] == 64 and np.all(lam > 0)


def test_cluster_compares_the_subspace(hc):
    ev = np.r_[[1.0, 1.0, 1.0], 2.0 + 0.25 * np.arange(147)]
    S = with_spectrum(ev, 2)
    tol = bound(S)
    lam, modes, st = host_modes(hc, S, 6)
    check_pairs(S, lam, modes, st, tol)
    _, V = reference(S)
    sine = subspace_sine(modes[:3].T, V[:, :3])
    print("cluster: subspace sine %.3g" % sine)
    assert sine <= 10 * TOLERANCE + tol
    for i in range(3, 6):   # the simple eigenvalues behind it: the vectors themselves
        assert abs(modes[i] @ V[:, i]) >= 1.0 - 1e-12


def test_indefinite_smallest_magnitude_is_negative(hc):
    ev = np.r_[-0.5, 1.0 + 0.5 * np.arange(80), -3.25 - 0.5 * np.arange(49)]   # no two of equal magnitude
    S = with_spectrum(ev, 3)
    tol = bound(S)
    lam, modes, st = host_modes(hc, S, 6)
    check_pairs(S, lam, modes, st, tol)
    assert lam[0] < 0 and abs(lam[0] + 0.5) <= tol * 0.5 and lam[1] > 0
    assert np.all(np.diff(np.abs(lam)) >= 0)


def test_full_space_first_rayleigh_ritz_is_exact(hc):
    S = with_spectrum(1.0 + np.arange(18.0), 4)
    tol = bound(S)
    lam, modes, st = host_modes(hc, S, 18)
    check_pairs(S, lam, modes, st, tol)
    assert st["iterations"] == 1 and st["block"] == 18


def test_near_singular(hc):
    ev = np.r_[1e-7, 1.0 + np.arange(99.0)]   # ||S|| = 100: the first eigenvalue sits at 1e-9 ||S||
    S = with_spectrum(ev, 5)
    tol = bound(S, None)
    lam, modes, st = host_modes(hc, S, 2)
    w, V = reference(S)
    check_pairs(S, lam, modes, st, tol, eigenvalues=False)
    ratio, want = lam[0] / lam[1], w[0] / w[1]
    print("near-singular: lambda_1 / lambda_2 = %.6g against %.6g" % (ratio, want))
    assert abs(ratio - want) <= tol * abs(want)
    assert abs(modes[0] @ V[:, 0]) >= 1.0 - 1e-12


def test_cap_reached_returns_the_last_ritz_values(hc):
    S = with_spectrum(10.0 ** (np.arange(200) / 20.0), 1)
    lam, modes, st = host_modes(hc, S, 6, max_iterations=1)
    assert st["iterations"] == 1 and st["converged"] < 6 and st["residual_max"] > TOLERANCE
    w, _ = reference(S)
    # Ritz values of S^-1 on a 64-dimensional space: each lies above the eigenvalue of S of the same rank
    assert np.all(lam >= w[:6] * (1 - 1e-9)) and np.all(np.diff(lam) >= 0) and np.all(np.isfinite(modes))


def test_same_bits_and_seed(hc):
    S = with_spectrum(1.0 + np.arange(100.0), 6)
    a = host_modes(hc, S, 4)
    b = host_modes(hc, S, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = host_modes(hc, S, 4, seed=7)
    assert not np.array_equal(a[1], c[1])
    assert np.max(np.abs(a[0] - c[0]) / a[0]) <= bound(S)


def test_wrong_variant_padding_rows_return_the_artificial_eigenvalue(hc):
    """n = 100 leaves 28 padding rows; every true eigenvalue is >= 2, the identity of the padding block has 1"""
    S = with_spectrum(2.0 + np.arange(100.0), 7)
    lam, _, st = host_modes(hc, S, 3)
    assert abs(lam[0] - 2.0) <= bound(S) * 2.0
    wrong, _, _ = host_modes(hc, S, 3, pad_nonzero=True)
    print("padding started non-zero: eigenvalues %s" % wrong)
    assert abs(wrong[0] - 1.0) <= 1e-9 and abs(lam[0] - 1.0) > 0.5
