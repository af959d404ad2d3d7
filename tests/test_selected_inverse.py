"""Selected inverse of the reduced camera system (ba_amd/csrc/selinv.h), checked on the CPU through
libba_hostcheck.so: the host restatement of the k_selinv recursion, run on random tile-sparse symmetric
matrices, reproduces every tile of S^-1 on the factor's pattern, and its tile-product count is the
formula sum_J |R_J|^2 + nt."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u8p = ctypes.POINTER(ctypes.c_uint8)
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    if not hasattr(lib, "ba_hostcheck_selinv"):
        import __graft_entry__
        __graft_entry__.build()
        lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_selinv.restype = ctypes.c_int
    lib.ba_hostcheck_selinv_products.restype = ctypes.c_uint64
    lib.ba_hostcheck_tile_factor.restype = ctypes.c_uint64
    return lib


def selinv(hc, S):
    n = S.shape[0]
    nt = (n + 63) // 64
    S = np.ascontiguousarray(S, dtype=np.float64)
    sig = np.zeros((n, n))
    nzL = np.zeros(nt * nt, dtype=np.uint8)
    prod, lev = ctypes.c_uint64(), ctypes.c_uint32()
    rc = hc.ba_hostcheck_selinv(n, S.ctypes.data_as(dp), sig.ctypes.data_as(dp), nzL.ctypes.data_as(u8p),
                                ctypes.byref(prod), ctypes.byref(lev))
    assert rc == 0
    return sig, nzL.reshape(nt, nt), prod.value, lev.value


def block_matrix(nblk, D, pairs, border=0, neg=(), seed=0):
    """Symmetric matrix of nblk D x D pose blocks coupled by `pairs`, plus a dense border of `border` rows;
    strictly diagonally dominant (the un-pivoted L D L^T exists), rows in `neg` with a negative diagonal."""
    rng = np.random.default_rng(seed)
    n = nblk * D + border
    S = np.zeros((n, n))
    for a in range(nblk):
        B = rng.standard_normal((D, D))
        S[a * D:(a + 1) * D, a * D:(a + 1) * D] = B + B.T
    for a, b in pairs:
        if a == b:
            continue
        B = rng.standard_normal((D, D))
        S[a * D:(a + 1) * D, b * D:(b + 1) * D] = B
        S[b * D:(b + 1) * D, a * D:(a + 1) * D] = B.T
    if border:
        B = rng.standard_normal((border, n))
        S[nblk * D:, :] = B
        S[:, nblk * D:] = B.T
        S[nblk * D:, nblk * D:] = B[:, nblk * D:] + B[:, nblk * D:].T
    dom = np.abs(S).sum(1) - np.abs(np.diag(S))
    d = dom * (1.0 + rng.uniform(0.2, 1.0, n)) + 1.0
    sgn = np.ones(n)
    sgn[list(neg)] = -1.0
    S[np.arange(n), np.arange(n)] = sgn * d
    return S


def check(hc, S, tol=1e-12):
    n = S.shape[0]
    cond = np.linalg.cond(S)
    assert cond <= 1e6
    sig, nzL, prod, lev = selinv(hc, S)
    ref = np.linalg.inv(S)
    nt = nzL.shape[0]
    scale = np.abs(ref).max()
    covered = 0
    for i in range(nt):
        for k in range(i + 1):
            if not (i == k or nzL[i, k]):
                continue
            r0, r1, c0, c1 = 64 * i, min(64 * i + 64, n), 64 * k, min(64 * k + 64, n)
            blk, want = sig[r0:r1, c0:c1], ref[r0:r1, c0:c1]
            assert np.all(np.isfinite(blk))
            err = np.abs(blk - want).max() / scale
            assert err <= tol, "tile (%d, %d): %.3g" % (i, k, err)
            if i != k:  # the upper half is returned by symmetry
                assert np.array_equal(sig[c0:c1, r0:r1], blk.T)
            covered += 1
    # tile products: sum_J |R_J|^2 + nt
    m = np.array([int(nzL[j + 1:, j].sum()) for j in range(nt)], dtype=np.int64)
    assert prod == int((m * m).sum()) + nt
    assert prod == hc.ba_hostcheck_selinv_products(nt, np.ascontiguousarray(nzL.ravel()).ctypes.data_as(u8p))
    return nzL, prod, lev, covered


@pytest.mark.parametrize("nblk,w", [(50, 3), (61, 12)])
def test_banded_pattern(hc, nblk, w):
    pairs = [(a, a + d) for a in range(nblk) for d in range(1, w + 1) if a + d < nblk]
    S = block_matrix(nblk, 6, pairs, seed=nblk)
    nzL, prod, lev, covered = check(hc, S)
    assert covered > nzL.shape[0]  # off-diagonal tiles too


def test_arrow_with_straddling_border(hc):
    # 21 poses of 6 rows = 126 rows, then a 6-row calibration border: rows 126..131 straddle tiles 1 and 2
    nblk = 21
    pairs = [(a, a + 1) for a in range(nblk - 1)]
    S = block_matrix(nblk, 6, pairs, border=6, seed=3)
    assert S.shape[0] == 132
    nzL, _, _, _ = check(hc, S)
    assert nzL[2, 0] and nzL[2, 1]  # the border row tile is dense


def test_arrow_many_tiles(hc):
    nblk = 60
    S = block_matrix(nblk, 6, [], border=4, seed=4)
    check(hc, S)


def test_three_lap_revisit(hc):
    # 3 laps of 32 poses: neighbours along the route and pose i coupled to i + 32, i + 64
    P, lap = 96, 32
    pairs = [(a, a + 1) for a in range(P - 1)]
    pairs += [(a, a + lap) for a in range(P - lap) if a % 3 == 0]
    S = block_matrix(P, 6, pairs, seed=5)
    nzL, prod, lev, _ = check(hc, S)
    assert lev <= nzL.shape[0]


@pytest.mark.parametrize("seed", [6, 7])
def test_negative_pivots(hc, seed):
    nblk = 40
    pairs = [(a, a + d) for a in range(nblk) for d in (1, 2) if a + d < nblk]
    rng = np.random.default_rng(seed)
    neg = rng.choice(nblk * 6, 30, replace=False)
    S = block_matrix(nblk, 6, pairs, border=5, neg=neg, seed=seed)
    assert (np.linalg.eigvalsh(S) < 0).any()
    check(hc, S)


def test_disjoint_branches_share_a_level(hc):
    # two independent chains joined only through a border: their columns sit on common levels
    nblk = 64
    pairs = [(a, a + 1) for a in range(31)] + [(a, a + 1) for a in range(32, 63)]
    S = block_matrix(nblk, 6, pairs, border=6, seed=8)
    nzL, prod, lev, _ = check(hc, S)
    assert lev < nzL.shape[0]


def test_partial_single_tile(hc):
    S = block_matrix(7, 6, [(0, 3), (2, 6)], border=1, seed=9)
    assert S.shape[0] == 43
    check(hc, S)
