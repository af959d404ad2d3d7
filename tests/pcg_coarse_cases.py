"""Systems and references shared by tests/test_pcg_coarse_plan.py (host restatement) and tests/test_pcg_coarse_gpu.py
(device) for the two-level preconditioner of the PCG solve (ba_hip_pcg_options.coarse_aggregate): the aggregate size
of every family of pcg_cases.families(), the aggregation matrix Z in numpy, the componentwise bound on C = Z^T S Z
and a textbook two-level PCG whose iteration counts the solver is held to."""
import ctypes
import os

import numpy as np

import pcg_cases as pc

EPS = pc.EPS
COARSE_MAX = 1024

# aggregates that straddle tile boundaries (64 is no multiple of g D), g = 1, one aggregate for everything, the
# 6-row border straddling tiles 1 and 2, and a system inside one tile
FAMILY_G = {
    "banded_D6": 10,                 # D 6: aggregates of 60 rows
    "chain_D9": 4,                   # D 9: 36 rows
    "banded_D15": 3,                 # D 15: 45 rows
    "dense_border_many_tiles": 1,    # Z = I on the poses and on the border
    "revisit_3_laps": 96,            # one aggregate for all 96 poses
    "arrow_straddling_border": 10,   # 21 poses: the last aggregate holds one pose; border rows 126 .. 131
    "partial_single_tile": 3,        # 7 poses and a border of 1 inside one tile
}


def used_aggregate(nblk, D, K, g):
    """the smallest aggregate >= g whose coarse space fits COARSE_MAX"""
    while D * -(-nblk // g) + K > COARSE_MAX and g < nblk:
        g += 1
    return g


def aggregation(n, D, K, g):
    """Z (n x nc): rows 0 .. n - K in blocks of D (a short last block feeds the leading coarse parameters of its
    aggregate), g consecutive blocks per aggregate; the K border rows are coarse unknowns of their own."""
    npose = n - K
    nblk = -(-npose // D)
    g = used_aggregate(nblk, D, K, g)
    naggr = -(-nblk // g)
    nc = D * naggr + K
    Z = np.zeros((n, nc))
    for r in range(npose):
        Z[r, (r // D // g) * D + r % D] = 1.0
    for k in range(K):
        Z[npose + k, D * naggr + k] = 1.0
    return Z, g, naggr


def coarse_reference(S, Z):
    """(C, componentwise bound 2 n eps Z^T |S| Z); coarse unknowns without a fine row carry 1 on the diagonal"""
    C = Z.T @ S @ Z
    bound = 2 * S.shape[0] * EPS * (Z.T @ np.abs(S) @ Z)
    empty = np.flatnonzero(Z.sum(axis=0) == 0)
    C[empty, empty] = 1.0
    return C, bound


def block_jacobi_inverse(S, n, D, K):
    npose = n - K
    M = np.zeros_like(S)
    starts = [(s, min(D, npose - s)) for s in range(0, npose, D)] + ([(npose, K)] if K else [])
    for s, d in starts:
        M[s:s + d, s:s + d] = np.linalg.inv(S[s:s + d, s:s + d])
    return M


def textbook_pcg(S, b, D, K, tol, Z=None, max_it=None):
    """Plain PCG, preconditioned by the diagonal blocks (D x D, then K x K) plus, with Z, the additive coarse
    correction Z (Z^T S Z)^-1 Z^T; stops when the recurrence's residual passes tol ||b||.  Returns (x, iterations)."""
    n = S.shape[0]
    Minv = block_jacobi_inverse(S, n, D, K)
    if Z is not None:
        C, _ = coarse_reference(S, Z)
        Cinv = np.linalg.inv(C)
        apply = lambda r: Minv @ r + Z @ (Cinv @ (Z.T @ r))
    else:
        apply = lambda r: Minv @ r
    x = np.zeros(n)
    r = b.copy()
    z = apply(r)
    p = z.copy()
    rz = r @ z
    bb = b @ b
    for it in range(1, (max_it or 4 * n) + 1):
        q = S @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if r @ r <= tol * tol * bb:
            return x, it
        z = apply(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it


# ---- the host restatement (libba_hostcheck.so) ---------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)


def host_lib():
    if not os.path.exists(HOSTCHECK):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(HOSTCHECK)
    lib.ba_hostcheck_pcg.restype = ctypes.c_int
    lib.ba_hostcheck_pcg2.restype = ctypes.c_int
    lib.ba_hostcheck_pcg_coarse.restype = ctypes.c_int
    return lib


def host_pcg2(hc, S, b, D, K, tol, g, max_it=0, coarse=False):
    """ba_hostcheck_pcg2: (x, rc, stats); with `coarse` the stats carry C and C^-1"""
    n = S.shape[0]
    a = np.ascontiguousarray(np.tril(S))
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.full(n, np.nan)
    u = np.zeros(6, dtype=np.uint32)
    f = np.zeros(3)
    c = np.zeros(4, dtype=np.uint32)
    C = Cinv = None
    if coarse:
        nc = aggregation(n, D, K, g)[0].shape[1]
        C, Cinv = np.full((nc, nc), np.nan), np.full((nc, nc), np.nan)
    rc = hc.ba_hostcheck_pcg2(n, a.ctypes.data_as(dp), b.ctypes.data_as(dp), n - K, D, ctypes.c_double(tol), max_it, g,
                              x.ctypes.data_as(dp), u.ctypes.data_as(u32p), f.ctypes.data_as(dp), c.ctypes.data_as(u32p),
                              C.ctypes.data_as(dp) if coarse else None, Cinv.ctypes.data_as(dp) if coarse else None)
    st = dict(iterations=int(u[0]), converged=int(u[1]), replacements=int(u[2]), breakdown=int(u[3]), passes=int(u[4]),
              tiles=int(u[5]), rel_recurrence=f[0], rel_true=f[1], rhs_norm=f[2], aggregate_used=int(c[0]),
              coarse_unknowns=int(c[1]), aggregates=int(c[2]), C=C, Cinv=Cinv)
    return x, rc, st
