"""Multi-RHS solves with the kept factor (ba_amd/csrc/factorsolve.h), checked on the CPU through
libba_hostcheck.so: the host restatement of the forward pass (k_joint_fsolve / k_joint_epilogue seeded with every
tile row) and of its backward mirror (k_fsol_bsolve / k_fsol_bepilogue) reproduces numpy.linalg.solve on the
cases of factor_solve_cases.py within both of its bounds, the levels and tile-product counts equal a numpy
restatement of the mirror plan, and three deliberately wrong variants of the restatement fail the same checks."""
import ctypes
import os

import numpy as np
import pytest

import factor_solve_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
dp = ctypes.POINTER(ctypes.c_double)
RIGHT, NO_SIGNS, UNTRANSPOSED, DROP_CHUNK = 0, 1, 2, 3   # FactorSolveVariant


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_factor_solve.restype = ctypes.c_int
    return lib


def host_solve(hc, S, B, tile_map=None, variant=RIGHT):
    """(X, nzL, backward level per tile column, (forward, backward) levels, (forward, backward) products)"""
    n, m = B.shape
    nt = (n + 63) // 64
    S = np.ascontiguousarray(S, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    tm = None if tile_map is None else np.ascontiguousarray(tile_map, dtype=np.uint8)
    X = np.zeros((n, m))
    nzL = np.zeros((nt, nt), dtype=np.uint8)
    blev = np.zeros(nt, dtype=np.uint32)
    lev = np.zeros(2, dtype=np.uint32)
    prod = np.zeros(2, dtype=np.uint64)
    rc = hc.ba_hostcheck_factor_solve(n, S.ctypes.data_as(dp), None if tm is None else tm.ctypes.data_as(u8p), m,
                                      B.ctypes.data_as(dp), variant, X.ctypes.data_as(dp), nzL.ctypes.data_as(u8p),
                                      blev.ctypes.data_as(u32p), lev.ctypes.data_as(u32p), prod.ctypes.data_as(u64p))
    assert rc == 0
    return X, nzL, blev, lev, prod


def _run(hc, name, m, kind, variant=RIGHT):
    c, S, _, tmap = fc.case(name)
    return host_solve(hc, S, fc.rhs(name, m, kind), tmap, variant)


@pytest.mark.parametrize("name,m,kind", fc.instances())
def test_restatement_against_numpy(hc, name, m, kind):
    X = _run(hc, name, m, kind)[0]
    fc.check_solution(name, m, kind, X)


@pytest.mark.parametrize("name", fc.CASES)
def test_levels_and_products_match_the_mirror_plan(hc, name):
    c = fc.case(name)[0]
    m = 130
    _, nzL, blev, lev, prod = _run(hc, name, m, "random")
    assert np.array_equal(nzL != 0, c.nzL != 0)
    fl, bl, fprod, bprod, _ = fc.mirror_plan(c.nzL, m)
    assert np.array_equal(blev, bl)
    assert lev[0] == fl.max() + 1 and lev[1] == bl.max() + 1
    assert prod[0] == fprod and prod[1] == bprod
    # every source of a column is finished one level earlier at the latest
    for j in range(c.nt):
        for i in range(j + 1, c.nt):
            if c.nzL[i, j]:
                assert blev[i] < blev[j]


def test_case_shapes_reach_their_edges():
    """the cases are what the module docstring says they are"""
    c = fc.case("dense6")[0]
    chunks = fc.mirror_plan(c.nzL, 1)[4]
    assert chunks[0] == 2 and int(c.nzL[1:, 0].sum()) == fc.CHUNK + 1   # a full chunk and a chunk of one
    assert fc.case("one18")[0].nt == 1 and fc.case("one18")[0].n == 18
    assert fc.case("two")[0].nzL[1, 0]
    assert any(fc.case(n)[0].n % 64 for n in fc.CASES) and (fc.case("dense6neg")[0].sgn < 0).any()
    b = fc.case("branches")[0].nzL
    assert not b[3:, :3].any() and b[2, 0] and b[5, 3]
    lone = fc.case("lone")[0].nzL
    assert not lone[2, :2].any() and not lone[3, 2]
    a = fc.case("arrow")
    first = a[0].n - 70
    assert first // 64 == a[0].nt - 2 and first % 64 and not a[1][first - 1, :64].any() and a[1][first, :64].all()
    sup = fc.case("superset")
    assert sup[3].sum() > (sup[0].nzL != 0).sum() - 1 and not sup[1][128:, :64].any()
    assert {m for _, m, _ in fc.instances()} >= set(fc.COLUMNS)


def _fails(name, m, kind, X):
    with pytest.raises(AssertionError):
        fc.check_solution(name, m, kind, X)


def test_wrong_variant_without_signs_fails(hc):
    X = _run(hc, "dense6neg", 65, "random", NO_SIGNS)[0]
    _fails("dense6neg", 65, "random", X)
    # ... and the signs are all that differs: on a positive definite case the variant is the computation
    assert np.array_equal(_run(hc, "dense6", 65, "random", NO_SIGNS)[0], _run(hc, "dense6", 65, "random")[0])


def test_wrong_variant_untransposed_fails(hc):
    for name in ("two", "dense6"):
        _fails(name, 65, "random", _run(hc, name, 65, "random", UNTRANSPOSED)[0])


def test_wrong_variant_dropped_second_chunk_fails(hc):
    _fails("dense6", 65, "random", _run(hc, "dense6", 65, "random", DROP_CHUNK)[0])
    # a column with at most kJointChunk sources has no second chunk: band3 is untouched by the variant
    assert np.array_equal(_run(hc, "band3", 65, "random", DROP_CHUNK)[0], _run(hc, "band3", 65, "random")[0])
