"""Matrices and assertions for the tile-sparse L D L^T factor (k_chol.hip), numpy only.

Shared by test_tile_factor.py (the CPU soundness gate: a plain float64 reference passes, mutated factors fail)
and test_tile_factor_gpu.py (the device factor through Engine.tile_solve under every kernel variant).

A case is a symmetric matrix held as 64x64 tiles (lower tile pairs only), built with the diagonal-dominance
recipe of test_selected_inverse.block_matrix at tile granularity, a right-hand side, three probe vectors and
the tile map handed to the factorisation.  The assertions are the componentwise backward-error bounds of an
un-pivoted Cholesky / L D L^T factorisation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
theorems 10.3 and 10.4; they hold for any order of summation and do not depend on the condition number),
evaluated in np.longdouble, tile by tile, in O(n^2) per vector:

    factor   |A v - L D L^T v|  <=  gamma_(n+1)  |L| |L^T| |v|     row by row, three probes v
    solve    |b - A x|          <=  gamma_(3n+1) |L| |L^T| |x|     row by row
    pattern  nzL == boolean symbolic elimination; every tile below the diagonal outside nzL is exactly zero
    signs    dsgn is +-1 and equals the sign of A's diagonal (congruent to a strictly diagonally dominant
             matrix, so that is the inertia)
    repeat   (caller) a second run returns the same bits

u = 2^-53, gamma_k = k u / (1 - k u).  L is rebuilt from the sub-diagonal tiles of the returned storage and
L_JJ = (linvT_J^T)^-1 by a 64x64 triangular inversion in long double.  The pass condition is ratio < 1.

Which (size, sign, grading) combinations a family runs: the four tile counts up to 5 run the full product
4 signs x {plain, graded}.  From 24 tiles on one solve costs a dense n x n upload and download plus O(n^2)
long-double work, so there every size runs ONE sign and grading, rotated with the family and the size (a
Latin arrangement): over the families every sign and both gradings meet every large size, and one family
x variant case stays at a few seconds.
"""
import numpy as np

NB = 64
U = 2.0 ** -53
LD = np.longdouble


def gamma(k):
    return LD(k) * LD(U) / (LD(1) - LD(k) * LD(U))


# ---- sizes: (tile count, n) -- the smallest that reach each branch of cholesky_solve ---------------------
SIZES = [
    (1, 7),       # one partial tile: only the tile-0 factor packet, identity padding from row 7
    (1, 64),      # one full tile, no padding
    (2, 100),     # one sub-diagonal tile, n ends inside the last tile
    (5, 320),     # KOUT = 4 (default) / 3: a second, ragged outer panel; one next-panel update, no bulk update
    (24, 1536),   # KOUT = 4, 128-path threshold lowered to 16: a_end = 8 leaves m = 16 (even) for k_update128
    (25, 1570),   # ... m = 17: the odd last tile row rides along as 64-tiles; n = 64 * 25 - 30 ends mid-tile
    (33, 2095),   # KOUT = 16: one look-ahead round (a_end = 32 < 33), ragged last panel of one tile; mid-tile n
    (41, 2624),   # KOUT = 16: two look-ahead rounds, ragged last panel of 9 tiles; KOUT = 8: five rounds
    (48, 3072),   # KOUT = 16 with the 128-path at threshold 16: m = 48 - 32 = 16 (even)
    (49, 3073),   # ... m = 17 (odd last tile row), and the last tile holds ONE row
]
SMALL_NT = 5      # up to here: the full sign x grading product
SIGNS = ["spd", "every7", "trailing", "onecol"]


def neg_rows(sign, nt, n):
    if sign == "spd":
        return np.zeros(0, dtype=np.int64)
    if sign == "every7":
        return np.arange(6, n, 7)
    if sign == "trailing":       # the quasi-definite shape of the dense-solve test
        return np.arange(n // 2, n)
    if sign == "onecol":         # one tile column: its panel takes the generic path, the others the fast path
        c = nt // 2
        return np.arange(NB * c, min(NB * c + NB, n), 3)
    raise KeyError(sign)


# ---- families: lower tile pairs (i, j, kind), kind 'd' dense or 'f' a few entries -------------------------
def _band(nt, w):
    return [(i, i - d, "f" if d == 2 else "d") for i in range(nt) for d in range(1, w + 1) if i - d >= 0]


def _random_tiles(nt, seed):
    rng = np.random.default_rng(1000 + seed)
    out = []
    for i in range(nt):
        for j in range(i):
            r = rng.random()
            if r < 0.15:
                out.append((i, j, "d" if r < 0.09 else "f"))
    return out


def family_tiles(name, nt):
    """(tile pairs, declared map or None).  None: the map is the pattern itself."""
    full = np.tril(np.ones((nt, nt), dtype=np.uint8))
    if name == "dense":
        return [(i, j, "d") for i in range(nt) for j in range(i)], None
    if name == "band1":
        return _band(nt, 1), None
    if name == "band3":
        return _band(nt, 3), None
    if name == "arrow":          # band 1 + two dense last tile rows: no fill
        p = {(i, j): k for i, j, k in _band(nt, 1)}
        for i in (nt - 2, nt - 1):
            for j in range(max(i, 0)):
                p[(i, j)] = "d"
        return [(i, j, k) for (i, j), k in sorted(p.items()) if i >= 0], None
    if name == "reverse_arrow":  # dense first tile column + band 1: fills completely
        p = {(i, j): k for i, j, k in _band(nt, 1)}
        for i in range(1, nt):
            p[(i, 0)] = "d"
        return [(i, j, k) for (i, j), k in sorted(p.items())], None
    if name == "blockdiag":      # blocks of 3 tiles + one far coupling: tile columns with nothing below the diagonal
        p = [(i, j, "d") for i in range(nt) for j in range(i) if i // 3 == j // 3]
        if nt > 3:
            p.append((nt - 1, 0, "f"))
        return p, None
    if name == "loop":           # band 1 + tile (nt - 1, 0): fill along the last row
        p = _band(nt, 1)
        if nt > 2:
            p.append((nt - 1, 0, "d"))
        return p, None
    if name == "lone1":          # (i odd, j even): every 128x128 block of k_update128 has exactly one live tile
        return [(i, j, "d") for i in range(1, nt, 2) for j in range(0, i, 2)], None
    if name == "lone2":          # (i odd, any j): the two lower tiles of every block
        return [(i, j, "d" if j % 2 == 0 else "f") for i in range(1, nt, 2) for j in range(i)], None
    if name == "random_a":
        return _random_tiles(nt, 1), None
    if name == "random_b":
        return _random_tiles(nt, 2), None
    if name == "superset":       # a band-1 matrix declared dense: declared tiles that hold only zeros
        return _band(nt, 1), full
    raise KeyError(name)


FAMILIES = ["dense", "band1", "band3", "arrow", "reverse_arrow", "blockdiag", "loop", "lone1", "lone2",
            "random_a", "random_b", "superset"]


def combos(family, sizes=None):
    """The (nt, n, sign, graded) instances of a family (see the module docstring)."""
    f = FAMILIES.index(family)
    out = []
    for s, (nt, n) in enumerate(SIZES):
        if sizes is not None and nt not in sizes:
            continue
        if nt <= SMALL_NT:
            out += [(nt, n, sg, g) for sg in SIGNS for g in (False, True)]
        else:
            out.append((nt, n, SIGNS[(f + s) % 4], ((f + s) // 4 + s) % 2 == 1))
    return out


# ---- numpy symbolic elimination ---------------------------------------------------------------------------
def symbolic(tile_map):
    """Lower tile pattern of L from the lower tile map (diagonal always set): L(i, j) fills in when L(i, k)
    and L(j, k) are nonzero, k < j <= i."""
    nz = np.tril(np.asarray(tile_map) != 0)
    nt = nz.shape[0]
    nz[np.arange(nt), np.arange(nt)] = True
    for k in range(nt):
        r = np.nonzero(nz[k + 1:, k])[0] + k + 1
        if r.size:
            nz[np.ix_(r, r)] |= np.tril(np.ones((r.size, r.size), dtype=bool))
    return nz.astype(np.uint8)


# ---- the generator ------------------------------------------------------------------------------------------
class Case:
    pass


def make_case(nt, n, pairs, neg=(), graded=False, seed=0, tile_map=None, name=""):
    """Symmetric n x n matrix (n in (64 (nt - 1), 64 nt]) with the lower tile pairs `pairs`, strictly
    diagonally dominant before the optional grading G A G, G = diag(10^U(-3, 3)); rows `neg` carry a negative
    diagonal."""
    assert NB * (nt - 1) < n <= NB * nt
    rng = np.random.default_rng(seed)
    ext = lambda t: min(NB, n - NB * t)  # rows of tile row t
    tiles = {}
    for t in range(nt):
        B = rng.standard_normal((ext(t), ext(t)))
        tiles[(t, t)] = B + B.T
    for i, j, kind in pairs:
        if not (0 <= j < i < nt):
            continue
        if kind == "d":
            B = rng.standard_normal((ext(i), ext(j)))
        else:
            B = np.zeros((ext(i), ext(j)))
            k = min(6, B.size)
            B[rng.integers(0, ext(i), k), rng.integers(0, ext(j), k)] = rng.standard_normal(k)
        tiles[(i, j)] = B
    dom = np.zeros(n)
    for (i, j), B in tiles.items():
        a = np.abs(B)
        if i == j:
            dom[NB * i:NB * i + ext(i)] += a.sum(1) - np.diag(a)
        else:
            dom[NB * i:NB * i + ext(i)] += a.sum(1)
            dom[NB * j:NB * j + ext(j)] += a.sum(0)
    d = dom * (1.0 + rng.uniform(0.2, 1.0, n)) + 1.0
    sgn = np.ones(n)
    sgn[np.asarray(neg, dtype=np.int64)] = -1.0
    for t in range(nt):
        k = np.arange(ext(t))
        tiles[(t, t)][k, k] = (sgn * d)[NB * t:NB * t + ext(t)]
    if graded:
        g = 10.0 ** rng.uniform(-3.0, 3.0, n)
        for (i, j), B in tiles.items():
            B *= np.outer(g[NB * i:NB * i + ext(i)], g[NB * j:NB * j + ext(j)])
        for t in range(nt):  # exactly symmetric diagonal tiles
            tiles[(t, t)] = np.tril(tiles[(t, t)]) + np.tril(tiles[(t, t)], -1).T
    c = Case()
    c.name, c.nt, c.n, c.ld, c.tiles, c.sgn = name, nt, n, NB * nt, tiles, sgn
    c.b = rng.standard_normal(n) * (g if graded else 1.0)
    pat = np.zeros((nt, nt), dtype=np.uint8)
    for (i, j) in tiles:
        pat[i, j] = 1
    c.tile_map = pat if tile_map is None else np.ascontiguousarray(tile_map, dtype=np.uint8)
    c.nzL = symbolic(c.tile_map)
    V = np.zeros((c.ld, 3))
    V[:n] = rng.standard_normal((n, 3))
    V[:n, 2] /= (g if graded else 1.0)   # one probe that weighs the small-scale rows up
    c.V = V.astype(LD)
    c.AV = a_times(c, c.V)               # exact side of the factor bound: computed once per case
    return c


def family_case(family, nt, n, sign, graded):
    pairs, tmap = family_tiles(family, nt)
    seed = 7919 * FAMILIES.index(family) + 101 * nt + 13 * SIGNS.index(sign) + int(graded)
    return make_case(nt, n, pairs, neg_rows(sign, nt, n), graded, seed, tmap,
                     "%s nt=%d n=%d %s%s" % (family, nt, n, sign, " graded" if graded else ""))


def lower_dense(c):
    """The lower triangle as the n x n row-major array the C entry takes."""
    a = np.zeros((c.ld, c.ld))
    for (i, j), B in c.tiles.items():
        a[NB * i:NB * i + B.shape[0], NB * j:NB * j + B.shape[1]] = B if i != j else np.tril(B)
    return np.ascontiguousarray(a[:c.n, :c.n])


def a_times(c, X):
    """A_pad X in long double, A_pad = diag(A, I): tile by tile."""
    X = np.asarray(X, dtype=LD)
    Y = np.zeros_like(X)
    Y[c.n:] = X[c.n:]
    for (i, j), B in c.tiles.items():
        Bl = B.astype(LD)
        r, q = slice(NB * i, NB * i + B.shape[0]), slice(NB * j, NB * j + B.shape[1])
        Y[r] += Bl @ X[q]
        if i != j:
            Y[q] += Bl.T @ X[r]
    return Y


# ---- triangular 64x64 inverses ----------------------------------------------------------------------------
def inv_lower(T, dtype):
    """Inverse of a lower-triangular tile by forward substitution, row by row, in `dtype`."""
    T = np.asarray(T, dtype=dtype)
    m = T.shape[0]
    X = np.zeros((m, m), dtype=dtype)
    for i in range(m):
        X[i, :i] = -(T[i, :i] @ X[:i, :i]) / T[i, i]
        X[i, i] = dtype(1) / T[i, i]
    return X


# ---- the assertions -------------------------------------------------------------------------------------------
class FactorCheckError(AssertionError):
    def __init__(self, which, msg):
        AssertionError.__init__(self, "%s: %s" % (which, msg))
        self.which = which


def _l_tiles(c, storage, linvT, nzL):
    T = {}
    for j in range(c.nt):
        T[(j, j)] = np.tril(inv_lower(np.asarray(linvT[j]).T, LD))
        for i in range(j + 1, c.nt):
            if nzL[i, j]:
                T[(i, j)] = storage[NB * i:NB * i + NB, NB * j:NB * j + NB].astype(LD)
    return T


def _lmul(T, X, transpose):
    Y = np.zeros_like(X)
    for (i, j), B in T.items():
        r, q = slice(NB * i, NB * i + NB), slice(NB * j, NB * j + NB)
        if transpose:
            Y[q] += B.T @ X[r]
        else:
            Y[r] += B @ X[q]
    return Y


def _ratio(res, bound):
    res, bound = np.abs(res), np.asarray(bound)
    if not np.all(np.isfinite(res)):
        return float("inf")
    zero = bound == 0
    if np.any(res[zero] != 0):
        return float("inf")
    return float(np.max(res[~zero] / bound[~zero])) if np.any(~zero) else 0.0


def check_factor(c, x, nzL, storage, linvT, dsgn):
    """Every assertion of the module docstring but `repeat`; returns (factor ratio, solve ratio)."""
    nt, n, ld = c.nt, c.n, c.ld
    nzL = np.asarray(nzL).reshape(nt, nt)
    storage = np.asarray(storage).reshape(ld, ld)
    # pattern
    if not np.array_equal(nzL != 0, c.nzL != 0):
        raise FactorCheckError("pattern", "%s: nzL differs from the symbolic elimination at tiles %s"
                               % (c.name, np.argwhere((nzL != 0) != (c.nzL != 0))[:4].tolist()))
    for i in range(nt):
        for j in range(i):
            if not c.nzL[i, j] and np.any(storage[NB * i:NB * i + NB, NB * j:NB * j + NB] != 0):
                raise FactorCheckError("pattern", "%s: tile (%d, %d) lies outside nzL but is not zero" % (c.name, i, j))
    # signs
    dsgn = np.asarray(dsgn)
    want = np.ones(ld)
    want[:n] = c.sgn
    if not np.array_equal(np.abs(dsgn), np.ones(ld)) or not np.array_equal(dsgn, want):
        bad = np.nonzero(dsgn != want)[0]
        raise FactorCheckError("signs", "%s: dsgn differs from the sign of A's diagonal at rows %s" % (c.name, bad[:6].tolist()))
    # factor and solve
    T = _l_tiles(c, storage, linvT, nzL)
    Ta = {k: np.abs(B) for k, B in T.items()}
    xp = np.zeros((ld, 1), dtype=LD)
    xp[:n, 0] = np.asarray(x, dtype=LD)
    X = np.concatenate([c.V, xp], axis=1)
    D = dsgn.astype(LD)[:, None]
    LDLtX = _lmul(T, D * _lmul(T, X, True), False)
    B = _lmul(Ta, _lmul(Ta, np.abs(X), True), False)
    rf = _ratio(c.AV - LDLtX[:, :3], gamma(n + 1) * B[:, :3])
    bp = np.zeros(ld, dtype=LD)
    bp[:n] = c.b
    rs = _ratio(bp - a_times(c, xp)[:, 0], gamma(3 * n + 1) * B[:, 3])
    if not rf < 1.0:
        raise FactorCheckError("factor", "%s: |A v - L D L^T v| is %.3g times gamma_(n+1) |L| |L^T| |v|" % (c.name, rf))
    if not rs < 1.0:
        raise FactorCheckError("solve", "%s: |b - A x| is %.3g times gamma_(3n+1) |L| |L^T| |x|" % (c.name, rs))
    return rf, rs


# ---- plain float64 reference: un-pivoted sign-L D L^T, blocked by 64 columns ------------------------------------
def reference_ldlt(c, skip_product=None, skip_rhs=None):
    """(x, nzL, storage, linvT, dsgn) like Engine.tile_solve(keep_factor=True).  Right-looking over tile
    columns; the trailing update is one numpy matmul over the tile rows of L's pattern.  Mutations for the
    soundness gate: skip_product = (i, k, J) leaves X_iJ D_J X_kJ^T out of tile (i, k); skip_rhs = J leaves
    the rhs row out of panel J's update."""
    nt, n, ld = c.nt, c.n, c.ld
    W = np.zeros((ld + 1, ld))
    W[:n, :n] = lower_dense(c)
    W[np.arange(n, ld), np.arange(n, ld)] = 1.0
    W[ld, :n] = c.b
    nzL = c.nzL
    dsgn = np.ones(ld)
    linvT = np.zeros((nt, NB, NB))
    for J in range(nt):
        c0, c1 = NB * J, NB * J + NB
        below = [i for i in range(J + 1, nt) if nzL[i, J]]
        idx = np.concatenate([np.arange(c0, c1)] + [np.arange(NB * i, NB * i + NB) for i in below] + [np.array([ld])])
        P = W[idx, c0:c1]
        s = np.ones(NB)
        for j in range(NB):
            piv = P[j, j]
            s[j] = -1.0 if piv < 0 else 1.0
            l = np.sqrt(abs(piv))
            P[j, j] = l
            P[j + 1:, j] /= l * s[j]
            if j + 1 < NB:
                P[j + 1:, j + 1:] -= np.outer(P[j + 1:, j], s[j] * P[j + 1:NB, j])
        P[:NB] = np.tril(P[:NB])
        W[idx, c0:c1] = P
        dsgn[c0:c1] = s
        linvT[J] = inv_lower(P[:NB], np.float64).T
        Xb = P[NB:]                      # the rows below the diagonal tile, rhs row last
        if below:
            ridx = idx[NB:]
            upd = (Xb * s) @ Xb[:-1].T
            if skip_rhs == J:
                upd[-1] = 0.0
            if skip_product is not None and skip_product[2] == J:
                a, b = below.index(skip_product[0]), below.index(skip_product[1])
                upd[NB * a:NB * a + NB, NB * b:NB * b + NB] = 0.0
            W[np.ix_(ridx, ridx[:-1])] -= upd
    for i in range(nt):                  # only the lower tiles are the factor
        W[NB * i:NB * i + NB, NB * i + NB:] = 0.0
    y = W[ld].copy()
    x = np.zeros(ld)
    for J in range(nt - 1, -1, -1):
        c0, c1 = NB * J, NB * J + NB
        x[c0:c1] = linvT[J] @ (y[c0:c1] - W[c1:ld, c0:c1].T @ x[c1:])
    return x[:n].copy(), nzL.copy(), W[:ld].copy(), linvT, dsgn
