"""The two-level preconditioner of the PCG solve (ba_amd/csrc/pcg.h, ba_hip_pcg_options.coarse_aggregate) without a
GPU, through libba_hostcheck.so: the coarse matrix C = Z^T S Z reads only the lower tiles of S's pattern and meets
the summation bound; pcg_host with the coarse correction converges to the true residual, in the number of iterations
of a textbook two-level PCG (+- 2), which is itself at most 0.6 / 0.5 of the block-Jacobi count where the
preconditioner claims to help; g = 1 on a block-diagonal system needs one iteration; an indefinite coarse matrix is
breakdown 4; the aggregate grows until the coarse space fits (and an absurd request is one aggregate, not an overflow); the
entry with coarse_aggregate = 0 forwards to the block-Jacobi one."""
import ctypes
import glob
import os

import numpy as np
import pytest

import pcg_cases as pc
import pcg_coarse_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "config1_*.npz")))
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)
FAMILIES = pc.families()


@pytest.fixture(scope="module")
def hc():
    return cc.host_lib()


pcg2 = cc.host_pcg2


def padded_store(S, garbage):
    """(nt, nz, A): the padded tile store of test_pcg_plan.test_spmv_reads_only_the_lower_tiles_of_the_pattern; with
    `garbage`, 1e30-sized values in the upper triangles of the diagonal tiles and in every tile outside the pattern"""
    n = S.shape[0]
    nt = (n + 63) // 64
    ld = 64 * nt
    nz = np.zeros((nt, nt), dtype=np.uint8)
    rng = np.random.default_rng(5)
    A = np.zeros((ld, ld))
    Sp = np.eye(ld)
    Sp[:n, :n] = S
    for i in range(nt):
        for j in range(nt):
            blk = Sp[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)]
            junk = rng.standard_normal((64, 64)) * 1e30 if garbage else np.zeros((64, 64))
            if i == j:
                nz[i, j] = 1
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = np.tril(blk) + np.triu(junk, 1)
            elif j < i and np.any(blk != 0.0):
                nz[i, j] = 1
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = blk
            else:
                A[64 * i:64 * (i + 1), 64 * j:64 * (j + 1)] = junk
    return nt, nz, np.ascontiguousarray(A)


@pytest.mark.parametrize("garbage", [False, True], ids=["clean", "garbage_outside_the_pattern"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_coarse_matrix_from_the_tiles_of_the_pattern(hc, name, garbage):
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    g = cc.FAMILY_G[name]
    Z, g_used, naggr = cc.aggregation(n, D, K, g)
    assert g_used == g
    nc = Z.shape[1]
    if name == "revisit_3_laps":
        assert naggr == 1
    if name in ("banded_D6", "chain_D9", "banded_D15"):
        assert 64 % (g * D) != 0 and n > g * D, "aggregates are meant to straddle tile boundaries"
    nt, nz, A = padded_store(S, garbage)
    C = np.full((nc, nc), np.nan)
    got = hc.ba_hostcheck_pcg_coarse(nt, np.ascontiguousarray(nz.ravel()).ctypes.data_as(u8p), A.ctypes.data_as(dp), n, n - K, D, g,
                                     C.ctypes.data_as(dp), None)
    assert got == nc
    ref, bound = cc.coarse_reference(S, Z)
    assert np.all(np.isfinite(C))
    assert np.all(np.abs(C - ref) <= bound), np.max(np.abs(C - ref) / np.maximum(bound, 1e-300))
    assert np.array_equal(C, C.T)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_coarse_matrix_does_not_depend_on_where_a_pose_ordering_puts_the_rows(hc, name):
    """The same values stored under a reversed and under a shuffled pose permutation (other tiles, other tile
    pattern) give the bits of natural order: every entry of C is one sum over the fine rows of its two coarse
    unknowns in natural order, not a combination of per-tile partial sums."""
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    g = cc.FAMILY_G[name]
    nblk = (n - K) // D
    nc = cc.aggregation(n, D, K, g)[0].shape[1]
    out = []
    for perm in (None, np.arange(nblk)[::-1], np.random.default_rng(3).permutation(nblk)):
        rows = np.arange(n)
        if perm is not None:
            for a in range(nblk):
                rows[perm[a] * D:(perm[a] + 1) * D] = np.arange(a * D, (a + 1) * D)   # position -> natural row
        Sp = S[np.ix_(rows, rows)]
        nt, nz, A = padded_store(Sp, True)
        C = np.full((nc, nc), np.nan)
        p32 = None if perm is None else np.ascontiguousarray(perm, dtype=np.uint32)
        got = hc.ba_hostcheck_pcg_coarse(nt, np.ascontiguousarray(nz.ravel()).ctypes.data_as(u8p), A.ctypes.data_as(dp), n, n - K, D,
                                         g, C.ctypes.data_as(dp), None if perm is None else p32.ctypes.data_as(u32p))
        assert got == nc
        out.append(C)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_two_level_pcg_host_converges_like_the_textbook(hc, name, tol):
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    g = cc.FAMILY_G[name]
    b = pc.rhs_for(S)
    Z, _, naggr = cc.aggregation(n, D, K, g)
    x, rc, st = pcg2(hc, S, b, D, K, tol, g, max_it=n, coarse=True)
    assert rc == 0 and st["converged"] == 1 and st["breakdown"] == 0, st
    assert (st["aggregate_used"], st["coarse_unknowns"], st["aggregates"]) == (g, Z.shape[1], naggr)
    rel = pc.assert_residual(S, b, x, tol)
    err = pc.assert_forward_error(S, b, x, tol)
    ref, bound = cc.coarse_reference(S, Z)
    C, Cinv = st["C"], st["Cinv"]
    assert np.all(np.abs(C - ref) <= bound)
    nc = C.shape[0]
    assert np.max(np.abs(C @ Cinv - np.eye(nc))) <= 8 * nc * cc.EPS * np.linalg.cond(C)
    assert np.array_equal(Cinv, Cinv.T)
    _, it_ref = cc.textbook_pcg(S, b, D, K, tol, Z)
    _, it_bj = cc.textbook_pcg(S, b, D, K, tol)
    print("%s tol %.0e g %d (%d coarse unknowns): %d iterations (textbook %d, block-Jacobi %d), residual %.2e, forward error %.2e"
          % (name, tol, g, Z.shape[1], st["iterations"], it_ref, it_bj, rel, err))
    assert abs(st["iterations"] - it_ref) <= 2


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_systems_need_at_most_0_6_of_the_block_jacobi_iterations(hc, path):
    g = np.load(path)
    U = np.triu(g["S_it0"])
    S = U + np.triu(U, 1).T
    b = g["rhs_it0"]
    n = S.shape[0]
    Z, _, _ = cc.aggregation(n, 6, 0, 4)
    _, it_bj = cc.textbook_pcg(S, b, 6, 0, 1e-10)
    _, it_ref = cc.textbook_pcg(S, b, 6, 0, 1e-10, Z)
    assert it_ref <= 0.6 * it_bj, (it_ref, it_bj)
    x, rc, st = pcg2(hc, S, b, 6, 0, 1e-10, 4, max_it=n)
    assert rc == 0 and st["converged"] == 1, st
    print("%s: %d iterations at 1e-10 with g = 4 (textbook %d, block-Jacobi %d)" % (os.path.basename(path), st["iterations"], it_ref, it_bj))
    assert abs(st["iterations"] - it_ref) <= 2
    pc.assert_residual(S, b, x, 1e-10)


def test_oracle_200_pose_scene_needs_at_most_half_the_block_jacobi_iterations(hc, oracle_lib):
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
    Z, _, _ = cc.aggregation(n, 6, 0, 10)
    assert Z.shape[1] == 120
    for tol in (1e-6, 1e-8):
        _, it_bj = cc.textbook_pcg(S, b, 6, 0, tol)
        _, it_ref = cc.textbook_pcg(S, b, 6, 0, tol, Z)
        assert it_ref <= 0.5 * it_bj, (tol, it_ref, it_bj)
        x, rc, st = pcg2(hc, S, b, 6, 0, tol, 10, max_it=n)
        assert rc == 0 and st["converged"] == 1, (tol, st)
        rel = pc.assert_residual(S, b, x, tol)
        print("oracle 200 poses, tol %.0e, g = 10: %d iterations (textbook %d, block-Jacobi %d), residual %.2e, step vs direct %.2e"
              % (tol, st["iterations"], it_ref, it_bj, rel, np.linalg.norm(x - o.delta_p()) / np.linalg.norm(o.delta_p())))
        assert abs(st["iterations"] - it_ref) <= 2


def test_g_1_on_a_block_diagonal_system_needs_one_iteration(hc):
    """Z = I and M_bj = S: M^-1 = 2 S^-1"""
    S = pc.block_diagonal()
    b = pc.rhs_for(S, 1)
    x, rc, st = pcg2(hc, S, b, 6, 0, 1e-10, 1)
    assert rc == 0 and st["converged"] == 1 and st["iterations"] == 1, st
    pc.assert_residual(S, b, x, 1e-10)


def test_indefinite_coarse_matrix_is_breakdown_4(hc):
    """every 6 x 6 block is the identity (the block-Jacobi part is fine), but with g = 1 the coarse matrix is S itself"""
    S, D, b = pc.indefinite_with_spd_blocks()
    x, rc, st = pcg2(hc, S, b, D, 0, 1e-12, 1, max_it=S.shape[0])
    assert rc == 4 and st["breakdown"] == 4 and st["converged"] == 0 and np.all(x == 0.0), st


def test_aggregate_grows_until_the_coarse_space_fits(hc):
    n = 1100
    rng = np.random.default_rng(7)
    S = np.diag(2.0 + rng.random(n))
    S += np.diag(0.5 * np.ones(n - 1), 1) + np.diag(0.5 * np.ones(n - 1), -1)
    b = pc.rhs_for(S, 5)
    x, rc, st = pcg2(hc, S, b, 1, 0, 1e-8, 1)
    assert rc == 0 and st["converged"] == 1, st
    assert st["aggregate_used"] == 2 and st["coarse_unknowns"] == 550 and st["aggregates"] == 550
    pc.assert_residual(S, b, x, 1e-8)


def test_an_absurd_aggregate_is_one_aggregate(hc):
    """g = 2^32 - 1 (what a negative command-line value becomes) must not wrap the aggregate count"""
    S, D, K = FAMILIES["arrow_straddling_border"]
    b = pc.rhs_for(S)
    x, rc, st = pcg2(hc, S, b, D, K, 1e-10, 0xFFFFFFFF, max_it=S.shape[0])
    assert rc == 0 and st["converged"] == 1, st
    assert (st["aggregate_used"], st["coarse_unknowns"], st["aggregates"]) == (21, D + K, 1), st
    pc.assert_residual(S, b, x, 1e-10)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_option_0_is_the_block_jacobi_solver_bit_for_bit(hc, name):
    """ba_hostcheck_pcg2 with coarse_aggregate = 0 forwards to ba_hostcheck_pcg: this only pins that the new entry
    keeps doing so.  The guard of the solver's bits with the option off is on the device
    (test_pcg_coarse_gpu.test_option_0_gives_the_bits_of_todays_callers_and_switches_without_finalize)."""
    S, D, K = FAMILIES[name]
    n = S.shape[0]
    b = pc.rhs_for(S)
    x2, rc2, st2 = pcg2(hc, S, b, D, K, 1e-10, 0, max_it=n)
    a = np.ascontiguousarray(np.tril(S))
    x = np.full(n, np.nan)
    u = np.zeros(6, dtype=np.uint32)
    f = np.zeros(3)
    rc = hc.ba_hostcheck_pcg(n, a.ctypes.data_as(dp), b.ctypes.data_as(dp), n - K, D, ctypes.c_double(1e-10), n,
                             x.ctypes.data_as(dp), u.ctypes.data_as(u32p), f.ctypes.data_as(dp))
    assert rc == rc2 == 0 and np.array_equal(x, x2)
    assert (int(u[0]), int(u[4]), f[1]) == (st2["iterations"], st2["passes"], st2["rel_true"])
    assert st2["coarse_unknowns"] == 0
