"""Systems and assertions shared by tests/test_pcg_plan.py (host restatement) and tests/test_pcg_gpu.py (device):
symmetric positive definite block matrices built like test_selected_inverse.block_matrix, the breakdown cases, and
the two bounds every converged solve has to meet."""
import numpy as np

from test_selected_inverse import block_matrix

EPS = np.finfo(np.float64).eps


def families():
    """name -> (S, D, K): np = n - K rows in pose blocks of D, then a dense border of K rows."""
    out = {}
    nblk = 40
    out["banded_D6"] = (block_matrix(nblk, 6, [(a, a + d) for a in range(nblk) for d in (1, 2) if a + d < nblk], seed=1), 6, 0)
    # 21 poses of 6 rows = 126 rows, then a 6-row border: rows 126..131 straddle tiles 1 and 2
    out["arrow_straddling_border"] = (block_matrix(21, 6, [(a, a + 1) for a in range(20)], border=6, seed=2), 6, 6)
    P, lap = 96, 32
    pairs = [(a, a + 1) for a in range(P - 1)] + [(a, a + k * lap) for a in range(P) for k in (1, 2) if a + k * lap < P]
    out["revisit_3_laps"] = (block_matrix(P, 6, pairs, seed=3), 6, 0)
    out["dense_border_many_tiles"] = (block_matrix(60, 6, [], border=4, seed=4), 6, 4)
    # 64 is no multiple of 9 or 15: blocks straddle tile boundaries
    out["chain_D9"] = (block_matrix(30, 9, [(a, a + 1) for a in range(29)], seed=5), 9, 0)
    out["banded_D15"] = (block_matrix(20, 15, [(a, a + d) for a in range(20) for d in (1, 3) if a + d < 20], seed=6), 15, 0)
    out["partial_single_tile"] = (block_matrix(7, 6, [(0, 3), (2, 6)], border=1, seed=9), 6, 1)
    return out


def rhs_for(S, seed=0):
    return np.random.default_rng(100 + seed).standard_normal(S.shape[0])


def assert_residual(S, b, x, tol):
    """converged => ||b - S x|| <= tol ||b|| + 2 n eps || |S||x| + |b| || (the second term: evaluating the residual)"""
    n = S.shape[0]
    res = np.linalg.norm(b - S @ x)
    bound = tol * np.linalg.norm(b) + 2 * n * EPS * np.linalg.norm(np.abs(S) @ np.abs(x) + np.abs(b))
    assert res <= bound, (res, bound)
    return res / np.linalg.norm(b)


def assert_forward_error(S, b, x, tol):
    """||x - x*|| / ||x*|| <= cond2(S) tol + 4.5 eps cond2(S)  (DESIGN section 8's constant for the direct solver)"""
    xs = np.linalg.solve(S, b)
    cond = np.linalg.cond(S)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    assert err <= cond * tol + 4.5 * EPS * cond, (err, cond, tol)
    return err


def block_diagonal(nblk=30, D=6, seed=11):
    return block_matrix(nblk, D, [], seed=seed)


def negative_block():
    """block 3 is negative definite (negative, dominant diagonal)"""
    nblk, D = 12, 6
    S = block_matrix(nblk, D, [(a, a + 1) for a in range(nblk - 1)], neg=range(3 * D, 4 * D), seed=12)
    return S, D


def indefinite_with_spd_blocks():
    """every 6 x 6 diagonal block is the identity, but the coupling 2 I between the poses 0 and 1 gives the
    eigenvalues 1 +- 2: S has the eigenvalue -1 (six times); b has components along those eigenvectors"""
    nblk, D = 10, 6
    S = np.eye(nblk * D)
    S[0:D, D:2 * D] = 2.0 * np.eye(D)
    S[D:2 * D, 0:D] = 2.0 * np.eye(D)
    for a in range(1, nblk - 1):
        S[a * D:(a + 1) * D, (a + 1) * D:(a + 2) * D] = 0.1 * np.eye(D)
        S[(a + 1) * D:(a + 2) * D, a * D:(a + 1) * D] = 0.1 * np.eye(D)
    b = rhs_for(S, 13)
    w, v = np.linalg.eigh(S)
    assert w[0] < -0.5 and abs(v[:, 0] @ b) > 1e-3
    return S, D, b
