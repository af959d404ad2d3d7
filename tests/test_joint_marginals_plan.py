"""Joint covariance of a row set without the selected inverse (ba_amd/csrc/jointcov.h), checked on the CPU
through libba_hostcheck.so: the host restatement of the k_joint kernels (forward substitution Y = L^-1 E over
the reach, then Y^T D Y) reproduces inv(S)[sel, sel] on random tile-sparse symmetric matrices, Y vanishes
outside the reach, the levels respect every dependency and the tile-product count is the formula
sum_{I in reach} |row(I) n reach| + |reach| per block of 64 columns."""
import ctypes
import os

import numpy as np
import pytest

from test_selected_inverse import block_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)
NONE = 0xFFFFFFFF
D = 6


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_joint_marginals.restype = ctypes.c_int
    return lib


def joint(hc, S, sel):
    n = S.shape[0]
    nt = (n + 63) // 64
    S = np.ascontiguousarray(S, dtype=np.float64)
    sel = np.ascontiguousarray(sel, dtype=np.uint32)
    m = len(sel)
    cov = np.zeros((m, m))
    Y = np.zeros((64 * nt, m))
    reach = np.zeros(nt, dtype=np.uint8)
    level_of = np.zeros(nt, dtype=np.uint32)
    nzL = np.zeros(nt * nt, dtype=np.uint8)
    prod, lev = ctypes.c_uint64(), ctypes.c_uint32()
    rc = hc.ba_hostcheck_joint_marginals(n, S.ctypes.data_as(dp), m, sel.ctypes.data_as(u32p), cov.ctypes.data_as(dp),
                                         Y.ctypes.data_as(dp), reach.ctypes.data_as(u8p), level_of.ctypes.data_as(u32p),
                                         nzL.ctypes.data_as(u8p), ctypes.byref(prod), ctypes.byref(lev))
    assert rc == 0
    return cov, Y, reach.astype(bool), level_of, nzL.reshape(nt, nt), prod.value, lev.value


def dense_ldl(S):
    """un-pivoted S = L D L^T with L carrying sqrt|pivot| and D = diag(+-1), in plain loops: structural zeros
    stay exact zeros"""
    n = S.shape[0]
    L = np.zeros((n, n))
    d = np.ones(n)
    for j in range(n):
        p = S[j, j] - (L[j, :j] * L[j, :j] * d[:j]).sum()
        d[j] = -1.0 if p < 0 else 1.0
        L[j, j] = np.sqrt(abs(p))
        L[j + 1:, j] = (S[j + 1:, j] - (L[j + 1:, :j] * d[:j]) @ L[j, :j]) / (d[j] * L[j, j])
    return L, d


def dense_forward(L, sel):
    """Y = L^-1 E row by row; a sum of exact zeros is an exact zero"""
    n = L.shape[0]
    Y = np.zeros((n, len(sel)))
    for r in range(n):
        e = (np.asarray(sel) == r).astype(np.float64)
        Y[r] = (e - L[r, :r] @ Y[:r]) / L[r, r]
    return Y


def expected_reach(nzL, tiles):
    nt = nzL.shape[0]
    inr = np.zeros(nt, dtype=bool)
    for t in tiles:
        j = int(t)
        while j < nt and not inr[j]:
            inr[j] = True
            below = np.nonzero(nzL[j + 1:, j])[0]
            j = j + 1 + int(below[0]) if len(below) else nt
    return inr


def pose_rows(poses, border=()):
    return [p * D + x for p in poses for x in range(D)] + list(border)


def check(hc, S, sel, tol=1e-12):
    n = S.shape[0]
    assert np.linalg.cond(S) <= 1e6
    cov, Y, reach, level_of, nzL, prod, lev = joint(hc, S, sel)
    nt = nzL.shape[0]
    ref = np.linalg.inv(S)[np.ix_(sel, sel)]
    err = np.abs(cov - ref).max() / np.abs(ref).max()
    assert err <= tol, err
    assert np.array_equal(cov, cov.T)
    # the reach: the union of the elimination-tree paths from the requested tiles
    assert np.array_equal(reach, expected_reach(nzL, sorted({s // 64 for s in sel})))
    # Y against a dense forward substitution, in which the rows outside the reach are exact zeros
    L, d = dense_ldl(S)
    Yd = dense_forward(L, sel)
    row_in = np.repeat(reach, 64)[:n]
    assert not Yd[~row_in].any()
    assert not Y[:n][~row_in].any() and not Y[n:].any()
    assert np.abs(Y[:n] - Yd).max() <= tol * max(1.0, np.abs(Yd).max())
    assert np.abs((Yd.T * d) @ Yd - ref).max() / np.abs(ref).max() <= tol
    # products per block of 64 columns and the level schedule
    ncb = (len(sel) + 63) // 64
    idx = np.nonzero(reach)[0]
    nsrc = sum(int(nzL[i, j]) for i in idx for j in idx if j < i)
    assert prod == ncb * (nsrc + len(idx))
    assert np.all(level_of[~reach] == NONE)
    for i in idx:
        src = [j for j in idx if j < i and nzL[i, j]]
        assert level_of[i] == (1 + max(level_of[j] for j in src) if src else 0)
    assert lev == int(level_of[reach].max()) + 1
    return cov, reach, nzL, lev


def banded(nblk, w, seed):
    pairs = [(a, a + k) for a in range(nblk) for k in range(1, w + 1) if a + k < nblk]
    return block_matrix(nblk, D, pairs, seed=seed)


@pytest.mark.parametrize("nblk,w", [(50, 3), (61, 12)])
def test_banded_reach_is_the_tail(hc, nblk, w):
    S = banded(nblk, w, nblk)
    nt = (S.shape[0] + 63) // 64
    for poses in ([0], [25], [1, nblk - 1], [10, 11], [nblk - 1]):  # pose 10: rows 60..65 straddle tiles 0 and 1
        sel = pose_rows(poses)
        _, reach, _, lev = check(hc, S, sel)
        t = min(sel) // 64
        assert np.array_equal(np.nonzero(reach)[0], np.arange(t, nt))
        assert lev == nt - t  # a chain


def test_arrow_with_straddling_border(hc):
    # 21 poses of 6 rows = 126 rows, then a 6-row border: rows 126..131 straddle tiles 1 and 2
    nblk = 21
    S = block_matrix(nblk, D, [(a, a + 1) for a in range(nblk - 1)], border=6, seed=3)
    border = list(range(126, 132))
    check(hc, S, pose_rows([4]))
    check(hc, S, pose_rows([0, 20], border))
    check(hc, S, border)
    check(hc, S, pose_rows([10, 20]))  # pose 10 straddles tiles 0 and 1


def test_three_lap_revisit(hc):
    P, lap = 96, 32
    pairs = [(a, a + 1) for a in range(P - 1)]
    pairs += [(a, a + lap) for a in range(P - lap) if a % 3 == 0]
    S = block_matrix(P, D, pairs, seed=5)
    check(hc, S, pose_rows([2]))
    check(hc, S, pose_rows([1, P - 1]))
    check(hc, S, pose_rows([10, 42, 53]))
    check(hc, S, pose_rows(range(0, P, 8)))  # 72 columns: two column blocks


@pytest.mark.parametrize("seed", [6, 7])
def test_negative_pivots(hc, seed):
    nblk = 40
    pairs = [(a, a + k) for a in range(nblk) for k in (1, 2) if a + k < nblk]
    rng = np.random.default_rng(seed)
    neg = rng.choice(nblk * D, 30, replace=False)
    S = block_matrix(nblk, D, pairs, border=5, neg=neg, seed=seed)
    assert (np.linalg.eigvalsh(S) < 0).any()
    n = S.shape[0]
    cov, _, _, _ = check(hc, S, pose_rows([0, 39], range(n - 5, n)))
    # D matters: without the signs the Gram product is another matrix
    L, d = dense_ldl(S)
    assert (d < 0).any()
    check(hc, S, pose_rows([int(neg[0]) // D]))


def test_disjoint_branches(hc):
    # two independent chains joined only through a border: a request in one chain never visits the other
    nblk = 64
    pairs = [(a, a + 1) for a in range(31)] + [(a, a + 1) for a in range(32, 63)]
    S = block_matrix(nblk, D, pairs, border=6, seed=8)
    n = S.shape[0]
    _, reach, nzL, _ = check(hc, S, pose_rows([40]))
    # chain A is poses 0..31 = rows 0..191 = tiles 0..2 exactly; chain B starts in tile 3
    assert not reach[:3].any() and reach[3:].all()
    _, reach, _, lev = check(hc, S, pose_rows([1]))
    assert reach[:3].all() and reach[-1] and not reach[3:-1].any()
    _, reach, _, lev2 = check(hc, S, pose_rows([1, 40], range(n - 6, n)))
    assert reach.all() and lev2 < int(reach.sum())  # the branches share levels


def test_partial_single_tile(hc):
    S = block_matrix(7, D, [(0, 3), (2, 6)], border=1, seed=9)
    assert S.shape[0] == 43
    check(hc, S, pose_rows([3]))
    check(hc, S, pose_rows([0, 6], [42]))


def test_selection_order_permutes_the_result(hc):
    S = banded(61, 12, 61)
    a = pose_rows([3, 30, 58])
    b = pose_rows([58, 3, 30])
    ca = joint(hc, S, a)[0]
    cb = joint(hc, S, b)[0]
    perm = [a.index(r) for r in b]
    assert np.abs(cb - ca[np.ix_(perm, perm)]).max() <= 1e-13 * np.abs(ca).max()
    assert np.array_equal(cb, cb.T)
