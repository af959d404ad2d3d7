"""The panel PCG (ba_amd/csrc/pcg_panel.h, ba_hip_pcg_panel_solve_system) without a GPU, through libba_hostcheck.so:
the cases of tests/pcg_panel_cases.py against textbook block-Jacobi PCG; pcg_panel_host — the restatement of the m
independent recurrences the kernels run in lock-step — on every system for m in {1, 6, 63, 64, 65, 130}: the two
bounds of pcg_cases per column, the zero column, the iteration counts of the single-column restatement, bitwise
independence of a column from its neighbours and from its place; the panel product against numpy; and three
deliberately wrong variants that these checks must catch."""
import ctypes
import os

import numpy as np
import pytest

import pcg_cases as pc
import pcg_panel_cases as pp
from test_pcg_plan import lower_tiles, pcg as pcg_single

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)
SYSTEMS = pp.systems()
RIGHT, WRONG_FROZEN_UPDATED, WRONG_DIAG_UPPER, WRONG_SHARED_ALPHA = 0, 1, 2, 3


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB) or not hasattr(ctypes.CDLL(LIB), "ba_hostcheck_pcg_panel"):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_pcg.restype = ctypes.c_int
    lib.ba_hostcheck_pcg_panel.restype = ctypes.c_int
    lib.ba_hostcheck_pcg_spmm.restype = ctypes.c_int
    return lib


def panel(hc, S, B, D, K, tol, max_it=0, variant=RIGHT, tile_map=None):
    """(X, rc, per-column dict of arrays, passes)"""
    n, m = B.shape
    s = np.ascontiguousarray(S, dtype=np.float64)
    b = np.ascontiguousarray(B, dtype=np.float64)
    x = np.full((n, m), np.nan)
    u = np.zeros(4 * m, dtype=np.uint32)
    f = np.zeros(2 * m)
    sc = np.zeros(4, dtype=np.uint32)
    tm = None if tile_map is None else np.ascontiguousarray(tile_map, dtype=np.uint8).ctypes.data_as(u8p)
    rc = hc.ba_hostcheck_pcg_panel(n, s.ctypes.data_as(dp), tm, m, b.ctypes.data_as(dp), n - K, D, ctypes.c_double(tol), max_it,
                                   variant, x.ctypes.data_as(dp), u.ctypes.data_as(u32p), f.ctypes.data_as(dp),
                                   sc.ctypes.data_as(u32p))
    u = u.reshape(m, 4)
    f = f.reshape(m, 2)
    st = dict(iterations=u[:, 0].copy(), converged=u[:, 1].copy(), breakdown=u[:, 2].copy(), replacements=u[:, 3].copy(),
              rel_true=f[:, 0].copy(), rel_recurrence=f[:, 1].copy(), passes=int(sc[0]), tiles=int(sc[1]), sources=int(sc[2]),
              chunks=int(sc[3]))
    return x, rc, st


def _solve(hc, name, m, tol, variant=RIGHT):
    S, D, K = SYSTEMS[name]
    B = pp.columns(name, S, m)
    X, rc, st = panel(hc, S, B, D, K, tol, max_it=S.shape[0], variant=variant)
    return S, D, K, B, X, rc, st


# ---- the cases themselves, against textbook PCG ----------------------------------------------------------------
def test_composite_iteration_counts_of_textbook_pcg():
    S, D, K = SYSTEMS["composite"]
    n = S.shape[0]
    assert n == 420 and D == 6 and K == 0
    cond = np.linalg.cond(S)
    assert 4.1e3 < cond < 4.3e3, cond
    rng = np.random.default_rng(7)
    unit = np.zeros(n)
    unit[7] = 1.0
    second = np.r_[np.zeros(pp.FIRST), rng.standard_normal(n - pp.FIRST)]
    dense = rng.standard_normal(n)
    for tol in pp.TOLS:
        for b, want in ((unit, 1), (second, 40), (dense, 41)):
            x, it = pp.textbook_pcg(S, D, b, tol)
            assert it == want, (tol, want, it)
            pc.assert_residual(S, b, x, tol)
            pc.assert_forward_error(S, b, x, tol)
        x, _ = pp.textbook_pcg(S, D, unit, tol)
        assert np.all(x[pp.FIRST:] == 0.0)
        x, _ = pp.textbook_pcg(S, D, second, tol)
        assert np.all(x[:pp.FIRST] == 0.0)


@pytest.mark.parametrize("name", sorted(pc.families()))
def test_family_columns_with_textbook_pcg(name):
    S, D, K = SYSTEMS[name]
    B = pp.columns(name, S, 6)
    for tol in pp.TOLS:
        for j in range(6):
            x, it = pp.textbook_pcg(S, D, B[:, j], tol)
            if not np.any(B[:, j]):
                assert it == 0 and np.all(x == 0.0)
                continue
            assert it <= 14, (name, j, it)
            pc.assert_residual(S, B[:, j], x, tol)
            pc.assert_forward_error(S, B[:, j], x, tol)


# ---- the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", pp.WIDTHS)
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_panel_host_meets_the_bounds_and_the_single_column_counts(hc, name, m):
    for tol in pp.TOLS:
        S, D, K, B, X, rc, st = _solve(hc, name, m, tol)
        assert rc == 0 and np.all(st["breakdown"] == 0) and np.all(st["converged"] == 1), st
        pp.assert_panel_bounds(S, pp.cond_of(name), B, X, tol, range(m))
        if m > 2:
            assert np.all(X[:, 2] == 0.0) and st["iterations"][2] == 0 and st["converged"][2] == 1
        # the single-column restatement (pcg_host) on the same column: one right-hand side per kind is enough for
        # the wide panels, the columns repeat with period 6 up to their random entries
        for j in (range(m) if m <= 6 else list(range(6)) + [m - 1]):
            _, rc1, s1 = pcg_single(hc, S, B[:, j], D, K, tol, max_it=S.shape[0])
            assert rc1 == 0 and s1["iterations"] == st["iterations"][j], (name, m, j, s1["iterations"], st["iterations"][j])
        if name == "composite" and m >= 2:
            assert st["iterations"][0] == 1 and st["iterations"][1] >= 40, st["iterations"][:6]
            assert np.all(X[pp.FIRST:, 0] == 0.0)
            if m > 4:
                assert st["iterations"][4] >= 40 and np.all(X[:pp.FIRST, 4] == 0.0)
        assert st["passes"] <= 2 * int(st["iterations"].max()) + 3


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_column_independence_is_bitwise(hc, name):
    S, D, K = SYSTEMS[name]
    n = S.shape[0]
    tol = 1e-10
    B = pp.columns(name, S, 63)
    X, rc, st = panel(hc, S, B, D, K, tol, max_it=n)
    assert rc == 0
    for j in (0, 1, 4, 5, 62):   # alone
        x1, rc1, s1 = panel(hc, S, B[:, [j]], D, K, tol, max_it=n)
        assert rc1 == 0 and np.array_equal(x1[:, 0], X[:, j]), j
        assert s1["iterations"][0] == st["iterations"][j] and s1["rel_true"][0] == st["rel_true"][j]
    perm = np.random.default_rng(1).permutation(63)   # permuted
    Xp, rcp, sp = panel(hc, S, B[:, perm], D, K, tol, max_it=n)
    assert rcp == 0 and np.array_equal(Xp, X[:, perm]) and np.array_equal(sp["iterations"], st["iterations"][perm])
    B65 = np.c_[pp.columns(name, S, 65, seed=1)[:, :2], B]   # widened across the 64-column boundary, and shifted by two
    Xw, rcw, sw = panel(hc, S, B65, D, K, tol, max_it=n)
    assert rcw == 0 and np.array_equal(Xw[:, 2:], X) and np.array_equal(sw["iterations"][2:], st["iterations"])


def test_breakdown_beside_healthy_columns(hc):
    S, D, B = pp.breakdown_system()
    n = S.shape[0]
    X, rc, st = panel(hc, S, B, D, 0, 1e-10, max_it=n)
    assert rc == 4
    assert st["breakdown"][0] == 1 and st["converged"][0] == 0 and np.all(np.isfinite(X[:, 0]))
    assert np.all(st["breakdown"][1:] == 0) and np.all(st["converged"][1:] == 1), st
    pp.assert_panel_bounds(S[60:, 60:], np.linalg.cond(S[60:, 60:]), B[60:, 1:], X[60:, 1:], 1e-10, range(5))
    assert np.all(X[:60, 1:] == 0.0)
    X2, rc2, st2 = panel(hc, S, B[:, 1:], D, 0, 1e-10, max_it=n)
    assert rc2 == 0 and np.array_equal(X2, X[:, 1:])


def test_iteration_cap_is_reported_per_column(hc):
    S, D, K = SYSTEMS["composite"]
    B = pp.columns("composite", S, 6)
    X, rc, st = panel(hc, S, B, D, K, 1e-10, max_it=5)
    assert rc == 0 and np.all(st["breakdown"] == 0)
    assert list(st["converged"]) == [1, 0, 1, 0, 0, 1] and list(st["iterations"]) == [1, 5, 0, 5, 5, 1], st


# ---- the product ------------------------------------------------------------------------------------------------
def _spmm_inputs(name, m):
    """as test_pcg_plan.test_spmv_reads_only_the_lower_tiles_of_the_pattern: garbage wherever the operator may not read"""
    S, D, K = SYSTEMS[name]
    n = S.shape[0]
    nt = (n + 63) // 64
    ld = 64 * nt
    nz = lower_tiles(S)
    rng = np.random.default_rng(5)
    A = np.full((ld, ld), np.nan)
    Sp = np.eye(ld)
    Sp[:n, :n] = S
    for i in range(nt):
        for j in range(i + 1):
            blk = Sp[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)]
            if i == j:
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = np.tril(blk) + np.triu(rng.standard_normal((64, 64)) * 1e30, 1)
            elif nz[i, j]:
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = blk
            else:
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = rng.standard_normal((64, 64)) * 1e30
    P = np.zeros((ld, m))
    P[:n] = rng.standard_normal((n, m))
    return S, n, nt, nz, np.ascontiguousarray(A), P


def _spmm(hc, nt, nz, A, P, variant=RIGHT):
    Q = np.full(P.shape, np.nan)
    out = np.zeros(2, dtype=np.uint32)
    rc = hc.ba_hostcheck_pcg_spmm(nt, np.ascontiguousarray(nz.ravel()).ctypes.data_as(u8p), A.ctypes.data_as(dp), P.shape[1],
                                  np.ascontiguousarray(P).ctypes.data_as(dp), Q.ctypes.data_as(dp), variant, out.ctypes.data_as(u32p))
    assert rc == 0
    return Q, int(out[0]), int(out[1])


@pytest.mark.parametrize("m", [1, 65])
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_spmm_against_numpy(hc, name, m):
    S, n, nt, nz, A, P = _spmm_inputs(name, m)
    Q, sources, chunks = _spmm(hc, nt, nz, A, P)
    tiles = int(np.tril(nz).sum())
    assert sources == 2 * tiles - nt        # every lower tile twice, the diagonal tiles once
    assert chunks >= nt
    ref = S @ P[:n]
    bound = 2 * n * pc.EPS * (np.abs(S) @ np.abs(P[:n]))
    assert np.all(np.abs(Q[:n] - ref) <= bound), np.max(np.abs(Q[:n] - ref) / bound)
    assert np.all(Q[n:] == 0.0)


# ---- the checks above catch wrong solvers ----------------------------------------------------------------------
def test_wrong_variant_frozen_columns_still_updated_is_caught(hc):
    S, D, K, B, X, rc, st = _solve(hc, "composite", 6, 1e-10, variant=WRONG_FROZEN_UPDATED)
    with pytest.raises(AssertionError):
        pp.assert_panel_bounds(S, pp.cond_of("composite"), B, X, 1e-10, range(6))
    x1, _, _ = panel(hc, S, B[:, [0]], D, K, 1e-10, max_it=S.shape[0], variant=WRONG_FROZEN_UPDATED)
    assert not np.array_equal(x1[:, 0], X[:, 0])   # ... and by the bitwise independence of a column


def test_wrong_variant_diagonal_upper_triangle_is_caught(hc):
    S, n, nt, nz, A, P = _spmm_inputs("banded_D6", 6)
    Q, _, _ = _spmm(hc, nt, nz, A, P, variant=WRONG_DIAG_UPPER)
    bound = 2 * n * pc.EPS * (np.abs(S) @ np.abs(P[:n]))
    assert not np.all(np.abs(Q[:n] - S @ P[:n]) <= bound)
    S, D, K, B, X, rc, st = _solve(hc, "banded_D6", 6, 1e-10, variant=WRONG_DIAG_UPPER)
    with pytest.raises(AssertionError):
        assert rc == 0 and np.all(st["converged"] == 1)
        pp.assert_panel_bounds(S, pp.cond_of("banded_D6"), B, X, 1e-10, range(6))


def test_wrong_variant_shared_alpha_is_caught(hc):
    """column 0 lives on the composite's second part, column 1 on its first, where the right step length is that of
    M = S: one iteration"""
    S, D, K = SYSTEMS["composite"]
    n = S.shape[0]
    B = np.random.default_rng(9).standard_normal((n, 2))
    B[:pp.FIRST, 0] = 0.0
    B[pp.FIRST:, 1] = 0.0
    X, rc, st = panel(hc, S, B, D, K, 1e-10, max_it=n, variant=WRONG_SHARED_ALPHA)
    _, _, s1 = pcg_single(hc, S, B[:, 1], D, K, 1e-10, max_it=n)
    assert s1["iterations"] == 1 and st["iterations"][1] != 1, st["iterations"]
    x1, _, _ = panel(hc, S, B[:, [1]], D, K, 1e-10, max_it=n, variant=WRONG_SHARED_ALPHA)
    assert not np.array_equal(x1[:, 0], X[:, 1])   # ... and column 1 depends on column 0
    Xr, rcr, sr = panel(hc, S, B, D, K, 1e-10, max_it=n)
    assert rcr == 0 and list(sr["iterations"]) == [40, 1]
