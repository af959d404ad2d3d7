"""The iterative reduced solve (ba_amd/csrc/pcg.h, ba_hip_set_reduced_solver) without a GPU, through
libba_hostcheck.so: the tile plan's symmetric product q = S v reads exactly the lower tiles of S's own pattern and
meets the standard summation bound; pcg_host — the restatement of the block-Jacobi PCG the kernels run, pass by pass —
converges to the true residual it reports, terminates within n steps, needs one step when M = S, and names its
breakdowns."""
import ctypes
import glob
import os

import numpy as np
import pytest

import pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "config1_*.npz")))
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)
FAMILIES = pc.families()


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    if not hasattr(lib, "ba_hostcheck_pcg"):
        import __graft_entry__
        __graft_entry__.build()
        lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_pcg.restype = ctypes.c_int
    lib.ba_hostcheck_pcg_spmv.restype = ctypes.c_uint32
    return lib


def pcg(hc, S, b, D, K, tol, max_it=0):
    n = S.shape[0]
    a = np.ascontiguousarray(np.tril(S))
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.full(n, np.nan)
    u = np.zeros(6, dtype=np.uint32)
    f = np.zeros(3)
    rc = hc.ba_hostcheck_pcg(n, a.ctypes.data_as(dp), b.ctypes.data_as(dp), n - K, D, ctypes.c_double(tol), max_it,
                             x.ctypes.data_as(dp), u.ctypes.data_as(u32p), f.ctypes.data_as(dp))
    st = dict(iterations=int(u[0]), converged=int(u[1]), replacements=int(u[2]), breakdown=int(u[3]), passes=int(u[4]),
              tiles=int(u[5]), rel_recurrence=f[0], rel_true=f[1], rhs_norm=f[2])
    return x, rc, st


def lower_tiles(S):
    n = S.shape[0]
    nt = (n + 63) // 64
    nz = np.zeros((nt, nt), dtype=np.uint8)
    for i in range(nt):
        for j in range(i + 1):
            if i == j or np.any(S[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] != 0.0):
                nz[i, j] = 1
    return nz


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_spmv_reads_only_the_lower_tiles_of_the_pattern(hc, name):
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    nt = (n + 63) // 64
    ld = 64 * nt
    nz = lower_tiles(S)
    rng = np.random.default_rng(5)
    # garbage everywhere; then only what the operator may read: off-diagonal tiles of the pattern in full, the lower
    # triangle of the diagonal tiles (the padding: identity)
    A = np.full((ld, ld), np.nan)
    Sp = np.eye(ld)
    Sp[:n, :n] = S
    for i in range(nt):
        for j in range(i + 1):
            blk = Sp[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)]
            if i == j:
                low = np.tril(blk) + np.triu(rng.standard_normal((64, 64)) * 1e30, 1)
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = low
            elif nz[i, j]:
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = blk
            else:
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = rng.standard_normal((64, 64)) * 1e30
    A = np.ascontiguousarray(A)
    v = np.zeros(ld)
    v[:n] = rng.standard_normal(n)
    q = np.full(ld, np.nan)
    visited = hc.ba_hostcheck_pcg_spmv(nt, np.ascontiguousarray(nz.ravel()).ctypes.data_as(u8p), A.ctypes.data_as(dp),
                                       v.ctypes.data_as(dp), q.ctypes.data_as(dp))
    assert visited == int(np.tril(nz).sum())
    if name in ("banded_D6", "revisit_3_laps", "dense_border_many_tiles", "chain_D9", "banded_D15"):
        assert visited < nt * (nt + 1) // 2, "the family is meant to have empty tiles"
    ref = S @ v[:n]
    bound = 2 * n * pc.EPS * (np.abs(S) @ np.abs(v[:n]))
    assert np.all(np.abs(q[:n] - ref) <= bound), np.max(np.abs(q[:n] - ref) / bound)
    assert np.all(q[n:] == 0.0)


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_pcg_host_converges_to_the_true_residual(hc, name, tol):
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    b = pc.rhs_for(S)
    x, rc, st = pcg(hc, S, b, D, K, tol, max_it=n)
    assert rc == 0 and st["converged"] == 1 and st["breakdown"] == 0, st
    assert st["iterations"] <= n
    rel = pc.assert_residual(S, b, x, tol)
    err = pc.assert_forward_error(S, b, x, tol)
    assert st["tiles"] == int(np.tril(lower_tiles(S)).sum())
    assert abs(st["rhs_norm"] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
    print("%s tol %.0e: %d iterations, %d replacements, residual %.2e (reported %.2e), forward error %.2e"
          % (name, tol, st["iterations"], st["replacements"], rel, st["rel_true"], err))


def test_block_diagonal_system_needs_one_iteration(hc):
    S = pc.block_diagonal()
    b = pc.rhs_for(S, 1)
    x, rc, st = pcg(hc, S, b, 6, 0, 1e-10)
    assert rc == 0 and st["converged"] == 1 and st["iterations"] == 1, st
    pc.assert_residual(S, b, x, 1e-10)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_systems_terminate_well_inside_n(hc, path):
    g = np.load(path)
    U = np.triu(g["S_it0"])
    S = U + np.triu(U, 1).T
    b = g["rhs_it0"]
    n = S.shape[0]
    x, rc, st = pcg(hc, S, b, 6, 0, 1e-10, max_it=n)
    assert rc == 0 and st["converged"] == 1, st
    assert st["iterations"] <= n
    pc.assert_residual(S, b, x, 1e-10)
    print("%s: %d of %d iterations at 1e-10 (plain numpy PCG: 64-73)" % (os.path.basename(path), st["iterations"], n))


def test_oracle_system_of_a_200_pose_scene(hc, oracle_lib):
    from ba_amd import scene
    from helpers import fill, gn_options
    po = oracle_lib
    sc = scene.make_scene(200, 20000, 10, lm_dim=1, seed=2)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    o = po.OracleBundleAdjuster(1, 6)
    o.Init(gn_options(po, apply_results=0))
    fill(o, sc, active=pa)
    o.Solve(1)
    U = np.triu(o.S())
    S = U + np.triu(U, 1).T
    b = o.rhs()
    n = S.shape[0]
    assert n == 1188
    numpy_counts = {1e-2: 4, 1e-4: 32, 1e-6: 66, 1e-8: 103, 1e-10: 122}
    for tol in (1e-2, 1e-4, 1e-6, 1e-8, 1e-10):
        x, rc, st = pcg(hc, S, b, 6, 0, tol, max_it=n)
        assert rc == 0 and st["converged"] == 1, (tol, st)
        assert st["iterations"] <= n
        rel = pc.assert_residual(S, b, x, tol)
        print("oracle 200 poses, tol %.0e: %d iterations (numpy: %d), %d replacements, residual %.2e, step vs direct %.2e"
              % (tol, st["iterations"], numpy_counts[tol], st["replacements"], rel,
                 np.linalg.norm(x - o.delta_p()) / np.linalg.norm(o.delta_p())))


def test_breakdowns_are_named_and_leave_a_finite_iterate(hc):
    S, D = pc.negative_block()
    x, rc, st = pcg(hc, S, pc.rhs_for(S, 2), D, 0, 1e-8)
    assert rc == 4 and st["breakdown"] == 3 and st["converged"] == 0 and np.all(x == 0.0), st
    S, D, b = pc.indefinite_with_spd_blocks()
    x, rc, st = pcg(hc, S, b, D, 0, 1e-12, max_it=S.shape[0])
    assert rc == 4 and st["breakdown"] == 1 and st["converged"] == 0 and np.all(np.isfinite(x)), st
    S, D, K = FAMILIES["banded_D6"]
    b = pc.rhs_for(S, 3)
    b[17] = np.nan
    x, rc, st = pcg(hc, S, b, D, K, 1e-8)
    assert rc == 4 and st["breakdown"] == 2 and st["converged"] == 0 and np.all(np.isfinite(x)), st


def test_iteration_cap_returns_a_descent_direction(hc):
    S, D, K = FAMILIES["revisit_3_laps"]
    b = pc.rhs_for(S, 4)
    x, rc, st = pcg(hc, S, b, D, K, 1e-10, max_it=3)
    assert rc == 0 and st["converged"] == 0 and st["breakdown"] == 0 and st["iterations"] == 3, st
    assert b @ x > 0.0
