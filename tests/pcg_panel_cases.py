"""Systems, right-hand sides and assertions shared by tests/test_pcg_panel_plan.py (host restatement) and
tests/test_pcg_panel_gpu.py (device) of the panel PCG (ba_amd/csrc/pcg_panel.h): the families of pcg_cases, a
composite system on which easy and hard columns share a panel, the system on which one column breaks down beside
healthy ones, and the two bounds of pcg_cases evaluated for every column of a panel at once."""
import functools

import numpy as np

import pcg_cases as pc

EPS = pc.EPS
WIDTHS = (1, 6, 63, 64, 65, 130)
TOLS = (1e-6, 1e-10)
FIRST = 180   # rows of the composite's first part


def composite():
    """diag(pcg_cases.block_diagonal() [180 rows: M = S, one iteration], kron(tridiag(-1, 2.001, -1) of order 40, I_6)
    [240 rows: block-Jacobi is a scaling, CG needs the 40 steps of its 40 distinct eigenvalues; cond 4.2e3])"""
    A = pc.block_diagonal()
    T = 2.001 * np.eye(40) - np.eye(40, k=1) - np.eye(40, k=-1)
    n1 = A.shape[0]
    assert n1 == FIRST
    S = np.zeros((n1 + 240, n1 + 240))
    S[:n1, :n1] = A
    S[n1:, n1:] = np.kron(T, np.eye(6))
    return S


@functools.lru_cache(maxsize=None)
def _systems():
    out = dict(pc.families())
    out["composite"] = (composite(), 6, 0)
    return out


def systems():
    """name -> (S, D, K) as pcg_cases.families()"""
    return _systems()


def columns(name, S, m, seed=0):
    """(n, m) right-hand sides, column j by j mod 6: 0 the unit column of row 0, 1 dense random, 2 (once, j = 2) zero,
    3 the unit column of the last row, 4 random — on the composite supported on the second part —, 5 random — on the
    composite the unit column of row 7 (first part)"""
    n = S.shape[0]
    rng = np.random.default_rng(200 + seed)
    B = rng.standard_normal((n, m))
    for j in range(m):
        k = j % 6
        if k == 0:
            B[:, j] = 0.0
            B[0, j] = 1.0
        elif j == 2:
            B[:, j] = 0.0
        elif k == 3:
            B[:, j] = 0.0
            B[n - 1, j] = 1.0
        elif name == "composite" and k == 4:
            B[:FIRST, j] = 0.0
        elif name == "composite" and k == 5:
            B[:, j] = 0.0
            B[7, j] = 1.0
    return B


@functools.lru_cache(maxsize=None)
def cond_of(name):
    return np.linalg.cond(systems()[name][0])


def assert_panel_bounds(S, cond, B, X, tol, which):
    """pcg_cases.assert_residual and assert_forward_error for the columns `which` of a panel: the same two bounds,
    with cond = cond2(S) and the reference solutions formed once"""
    n = S.shape[0]
    XS = np.linalg.solve(S, B)
    R = B - S @ X
    absx = np.abs(S) @ np.abs(X) + np.abs(B)
    worst = (0.0, 0.0)
    for j in which:
        nb = np.linalg.norm(B[:, j])
        if nb == 0.0:
            assert np.all(X[:, j] == 0.0), j
            continue
        res = np.linalg.norm(R[:, j])
        bound = tol * nb + 2 * n * EPS * np.linalg.norm(absx[:, j])
        assert res <= bound, (j, res, bound)
        err = np.linalg.norm(X[:, j] - XS[:, j]) / np.linalg.norm(XS[:, j])
        assert err <= cond * tol + 4.5 * EPS * cond, (j, err, cond, tol)
        worst = (max(worst[0], res / nb), max(worst[1], err))
    return worst


def textbook_pcg(S, D, b, tol, max_it=None):
    """Block-Jacobi PCG as in the textbooks (blocks of D rows, the last one shorter): (x, iterations); stops when the
    recurrence's ||r|| <= tol ||b||"""
    n = S.shape[0]
    Minv = np.zeros_like(S)
    for s in range(0, n, D):
        e = min(n, s + D)
        Minv[s:e, s:e] = np.linalg.inv(S[s:e, s:e])
    x = np.zeros(n)
    nb = np.linalg.norm(b)
    if nb == 0.0:
        return x, 0
    r = b.copy()
    z = Minv @ r
    p = z.copy()
    rz = r @ z
    for it in range(1, (max_it or n) + 1):
        q = S @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= tol * nb:
            return x, it
        z = Minv @ r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it or n


def breakdown_system():
    """(S, D, B): diag(the matrix of pcg_cases.indefinite_with_spd_blocks() [60 rows], banded_D6 [240 rows]).  Column 0
    is that helper's b on the first part: it breaks down with code 1 (p.Sp <= 0).  The other five columns are
    supported on the second part only: exactly decoupled from the first, they converge."""
    S1, D, b = pc.indefinite_with_spd_blocks()
    S2 = pc.families()["banded_D6"][0]
    n1, n2 = S1.shape[0], S2.shape[0]
    S = np.zeros((n1 + n2, n1 + n2))
    S[:n1, :n1] = S1
    S[n1:, n1:] = S2
    B = np.zeros((n1 + n2, 6))
    B[:n1, 0] = b
    B[n1:, 1:] = np.random.default_rng(300).standard_normal((n2, 5))
    B[n1:, 5] = 0.0
    B[n1 + 3, 5] = 1.0
    return S, D, B
