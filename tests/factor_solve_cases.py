"""Matrices, right-hand sides and assertions for the multi-RHS solve with the kept factor (factorsolve.h,
k_factorsolve.hip), numpy only.  Shared by test_factor_solve_plan.py (the host restatement through
libba_hostcheck.so) and test_factor_solve_gpu.py (the device through Engine.tile_factor_solve).

The tile patterns come from tile_factor_cases.py (the diagonal-dominance recipe, never graded: cond(S) stays
small, so the forward bound below stays at its floor); this module adds the shapes that reach each edge of the
substitution plan:

    one18      nt = 1, n = 18 (three 6-parameter poses): no source at all
    two        nt = 2: the smallest case with a source
    dense6     dense nt = 6: column 0 has 5 sources, kJointChunk = 4 -> a full chunk and a chunk of one
    dense6neg  ... with negative pivots every 7th row: D = +-1 in the backward pass
    band3      band of 3 tiles, n ends inside the last tile
    bandneg    band of 1 tile, the trailing half of the rows negative
    arrow      band 1 + a dense border of 70 rows that starts inside tile nt - 2 (it straddles a tile)
    branches   two disjoint blocks of 3 tiles: independent subtrees
    lone       tiles 0-1 and 1-3 coupled, tile 2 on its own
    superset   a band-1 matrix declared dense: declared tiles that hold only zeros

Bounds (u = eps = 2^-52):
    residual   ||B - S X||_F / (||S||_F ||X||_F) <= n eps   normwise backward error of a Cholesky-type solve without
               growth; independent of cond(S)
    forward    max|X - X_ref| / max|X_ref| <= max(1e-9, 4.5 eps cond(S))   (DESIGN.md section 8), asserted <= 1e-8
"""
import functools

import numpy as np

import tile_factor_cases as tf

EPS = np.finfo(np.float64).eps
NB = 64
CHUNK = 4   # kJointChunk


def _dense(nt):
    return [(i, j, "d") for i in range(nt) for j in range(i)]


def _arrow(nt, n, border):
    """band 1 plus a dense border of the last `border` rows"""
    c = tf.make_case(nt, n, tf.family_tiles("arrow", nt)[0], seed=4242, name="arrow")
    first = n - border
    t = first // NB
    assert first % NB != 0 and t == nt - 2, "the border must start inside tile nt - 2"
    for j in range(t - 1):       # rows of tile row t above the border keep only their band
        c.tiles[(t, j)][:first - NB * t] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case of tile_factor_cases, dense symmetric S, lower triangle, tile map or None)"""
    mk = tf.make_case
    tmap = None
    if name == "one18":
        c = mk(1, 18, [], seed=1, name=name)
    elif name == "two":
        c = mk(2, 100, _dense(2), seed=2, name=name)
    elif name == "dense6":
        c = mk(6, 370, _dense(6), seed=3, name=name)
    elif name == "dense6neg":
        c = mk(6, 384, _dense(6), neg=tf.neg_rows("every7", 6, 384), seed=4, name=name)
    elif name == "band3":
        c = mk(5, 300, tf.family_tiles("band3", 5)[0], seed=5, name=name)
    elif name == "bandneg":
        c = mk(5, 320, tf.family_tiles("band1", 5)[0], neg=tf.neg_rows("trailing", 5, 320), seed=6, name=name)
    elif name == "arrow":
        c = _arrow(6, 380, 70)
    elif name == "branches":
        c = mk(6, 384, [(i, j, "d") for i in range(6) for j in range(i) if i // 3 == j // 3], seed=7, name=name)
    elif name == "lone":
        c = mk(4, 250, [(1, 0, "d"), (3, 1, "d")], seed=8, name=name)
    elif name == "superset":
        full = np.tril(np.ones((4, 4), dtype=np.uint8))
        c = mk(4, 230, tf.family_tiles("band1", 4)[0], seed=9, tile_map=full, name=name)
        tmap = full
    else:
        raise KeyError(name)
    lower = tf.lower_dense(c)
    S = lower + np.tril(lower, -1).T
    return c, S, lower, tmap


CASES = ["one18", "two", "dense6", "dense6neg", "band3", "bandneg", "arrow", "branches", "lone", "superset"]
COLUMNS = [1, 63, 64, 65, 130]   # column-block edges


def rhs(name, m, kind="random"):
    """B (n x m).  kind: random; first / last: a single non-zero row, in the first / the last tile."""
    n = case(name)[0].n
    rng = np.random.default_rng(1 + 31 * CASES.index(name) + m)
    B = rng.standard_normal((n, m))
    if kind == "first":
        B[np.arange(n) != min(5, n - 1)] = 0.0
    elif kind == "last":
        B[np.arange(n) != n - 2] = 0.0
    elif kind != "random":
        raise KeyError(kind)
    return B


def instances():
    """(case, m, kind): every case with m = 65 (two column blocks, the second nearly empty), every m on the case
    with the chunk edge, the other m rotated over the cases, sparse right-hand sides at either end."""
    out = [(c, 65, "random") for c in CASES]
    out += [("dense6", m, "random") for m in COLUMNS if m != 65]
    out += [(c, [1, 63, 64, 130][i % 4], "random") for i, c in enumerate(CASES) if c != "dense6"]
    out += [(c, 3, k) for c in ("two", "dense6neg", "arrow", "lone") for k in ("first", "last")]
    return out


@functools.lru_cache(maxsize=None)
def forward_tol(name):
    tol = max(1e-9, 4.5 * EPS * np.linalg.cond(case(name)[1]))
    assert tol <= 1e-8, "case too ill-conditioned for the check: %g" % tol
    return tol


@functools.lru_cache(maxsize=None)
def reference(name, m, kind):
    X = np.linalg.solve(case(name)[1], rhs(name, m, kind))
    X.setflags(write=False)
    return X


def residual_ratio(S, B, X):
    """||B - S X||_F / (||S||_F ||X||_F) over n eps: passes below 1"""
    n = S.shape[0]
    if not np.all(np.isfinite(X)):
        return float("inf")
    return float(np.linalg.norm(B - S @ X) / (np.linalg.norm(S) * np.linalg.norm(X)) / (n * EPS))


def forward_err(X, Xref):
    if not np.all(np.isfinite(X)):
        return float("inf")
    return float(np.abs(X - Xref).max() / np.abs(Xref).max())


def check_solution(name, m, kind, X):
    """Both bounds of the module docstring against numpy.linalg.solve; returns (residual ratio, forward error)."""
    _, S, _, _ = case(name)
    B = rhs(name, m, kind)
    rr = residual_ratio(S, B, X)
    fe = forward_err(X, reference(name, m, kind))
    assert rr <= 1.0, "%s m=%d %s: residual is %.3g times n eps" % (name, m, kind, rr)
    assert fe <= forward_tol(name), "%s m=%d %s: forward error %.3g > %.3g" % (name, m, kind, fe, forward_tol(name))
    return rr, fe


# ---- numpy restatement of the two schedules -----------------------------------------------------------------
def mirror_plan(nzL, m):
    """(forward level per tile row, backward level per tile column, forward products, backward products, chunks per
    column of the backward pass) from the lower factor pattern."""
    nz = np.asarray(nzL) != 0
    nt = nz.shape[0]
    ncb = (m + 63) // 64
    fl = np.zeros(nt, dtype=np.int64)
    for i in range(nt):
        src = [j for j in range(i) if nz[i, j]]
        fl[i] = 1 + max(fl[j] for j in src) if src else 0
    bl = np.zeros(nt, dtype=np.int64)
    chunks = np.zeros(nt, dtype=np.int64)
    for j in range(nt - 1, -1, -1):
        src = [i for i in range(j + 1, nt) if nz[i, j]]
        bl[j] = 1 + max(bl[i] for i in src) if src else 0
        chunks[j] = (len(src) + CHUNK - 1) // CHUNK
    off = int(np.tril(nz, -1).sum())
    return fl, bl, ncb * (off + nt), ncb * (off + nt), chunks
