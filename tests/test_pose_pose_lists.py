"""Pose-pose half of the static structure (ba_amd/csrc/structure.h), checked on the CPU.

`ba_hostcheck_pose_pose_lists` runs the finalize steps of a graph without projections as the engine runs them
(`build_lists` for the opt ids, `build_pose_pose_lists`, `mark_pose_pose_tiles`) and then restates `k_pp_scatter` on the
host.  Here the result is compared with a brute-force sum written independently: for every residual slot
`[unary | binary | imu]` the blocks H11 / H12 / H22 and the gradients g1 / g2 are taken from the caller's `pp_h` / `pp_g` and
placed by opt id into a full symmetric matrix, masks zero rows and columns, and the lower storage is read off.  Index
logic only: the blocks are random.

`S` and the right-hand side must agree EXACTLY: an element of block (j, i) receives one addend per residual that ties
the two poses, and both sides add them in slot order starting from zero (the scatter entries of a pose are in slot
order; the brute force walks the slots), so every element sees the same additions in the same order.  Masked elements
are never written on the one side and zeroed on the other.

One behaviour is pinned, not derived: a binary or inertial residual with p1 == p2 contributes H11 and g1 only
(DESIGN.md section 8); the brute force states that rule in one line.
"""
import ctypes
import math

import numpy as np
import pytest

from helpers import hostcheck_lib

NONE = 0xFFFFFFFF
UNKNOWN_POSE = "pose-pose residual references an unknown pose"


@pytest.fixture(scope="module")
def hc():
    lib = hostcheck_lib()
    lib.ba_hostcheck_coupling_group_edges.restype = ctypes.c_uint64
    return lib


class Graph:
    def __init__(self, D, active, unary=(), binary=(), imu=(), priors=(), masks=None, K=0, perm=None):
        self.D, self.K = D, K
        self.active = np.asarray(active, dtype=np.uint8)
        self.P = len(self.active)
        self.unary = [int(p) for p in unary]
        self.binary = [(int(a), int(b)) for a, b in binary]
        self.imu = [(int(a), int(b)) for a, b in imu]
        self.priors = [list(q) for q in priors]
        self.masks = np.zeros(self.P, dtype=np.uint16)
        for p, m in (masks or {}).items():
            self.masks[p] = m
        self.perm = None if perm is None else np.asarray(perm, dtype=np.uint32)

    @property
    def Pact(self):
        return int(self.active.sum())

    @property
    def slots(self):
        """(p1, p2 or NONE) per slot [unary | binary | imu]"""
        return [(p, NONE) for p in self.unary] + self.binary + self.imu

    def natural_opt(self):
        nat = np.full(self.P, -1, dtype=np.int64)
        nat[self.active != 0] = np.arange(self.Pact)
        return nat

    def pose_opt(self):
        opt = self.natural_opt()
        if self.perm is not None:
            opt[opt >= 0] = self.perm[opt[opt >= 0]]
        return opt

    def with_(self, **kw):
        d = dict(D=self.D, active=self.active, unary=self.unary, binary=self.binary, imu=self.imu, priors=self.priors,
                 masks={p: int(m) for p, m in enumerate(self.masks) if m}, K=self.K, perm=self.perm)
        d.update(kw)
        return Graph(**d)


def _u32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.uint32).reshape(-1))


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _prior_csr(g):
    ptr = np.zeros(len(g.priors) + 1, dtype=np.uint32)
    ptr[1:] = np.cumsum([len(q) for q in g.priors])
    return ptr, _u32([p for q in g.priors for p in q])


def host_lists(hc, g, pp_h, pp_g):
    """-> (rc, message, dict of outputs)"""
    u32, dbl = ctypes.c_uint32, ctypes.c_double
    n = g.Pact * g.D + g.K
    ld = max(64, (n + 63) // 64 * 64)
    nt = ld // 64
    nres = len(g.slots)
    S, rhs = np.full((ld, ld), np.nan), np.full(ld, np.nan)
    tile_nz = np.full((nt, nt), 7, dtype=np.uint8)
    counts = np.zeros(5, dtype=np.uint32)
    pp_ptr = np.zeros(g.Pact + 1, dtype=np.uint32)
    pp_ent = np.zeros((max(2 * nres, 1), 4), dtype=np.uint32)
    msg = ctypes.create_string_buffer(128)
    perm = _u32([] if g.perm is None else g.perm)
    un = _u32(g.unary)
    b1, b2 = _u32([a for a, _ in g.binary]), _u32([b for _, b in g.binary])
    i1, i2 = _u32([a for a, _ in g.imu]), _u32([b for _, b in g.imu])
    qptr, qpose = _prior_csr(g)
    rc = hc.ba_hostcheck_pose_pose_lists(
        g.D, g.K, g.P, _ptr(g.active, ctypes.c_uint8), len(perm), _ptr(perm, u32), len(un), _ptr(un, u32),
        len(b1), _ptr(b1, u32), _ptr(b2, u32), len(i1), _ptr(i1, u32), _ptr(i2, u32),
        len(g.priors), _ptr(qptr, u32), _ptr(qpose, u32), _ptr(g.masks, ctypes.c_uint16), _ptr(pp_h, dbl), _ptr(pp_g, dbl),
        ld, _ptr(S, dbl), _ptr(rhs, dbl), _ptr(tile_nz, ctypes.c_uint8), _ptr(counts, u32), _ptr(pp_ptr, u32),
        _ptr(pp_ent, u32), msg, len(msg))
    return rc, msg.value.decode(), dict(S=S, rhs=rhs, tile_nz=tile_nz, counts=counts, pp_ptr=pp_ptr, pp_ent=pp_ent,
                                        n=n, ld=ld, nt=nt)


def random_blocks(g, seed):
    rng = np.random.default_rng(seed)
    nres = max(len(g.slots), 1)
    return rng.normal(size=(nres, 3, 15, 15)), rng.normal(size=(nres, 2, 15))


def brute_force(g, pp_h, pp_g):
    """-> (S as the lower storage holds it, n x n; rhs; tiles nt x nt; expected scatter entries per opt id)"""
    D, opt = g.D, g.pose_opt()
    n_p = g.Pact * D
    n = n_p + g.K
    ld = max(64, (n + 63) // 64 * 64)
    F, rhs = np.zeros((ld, ld)), np.zeros(ld)
    touched = np.zeros((ld, ld), dtype=bool)      # elements of the pattern of S
    entries = [[] for _ in range(g.Pact)]

    def blk(o):
        return slice(o * D, o * D + D)

    for s, (p1, p2) in enumerate(g.slots):
        o1 = opt[p1]
        o2 = opt[p2] if p2 != NONE and p2 != p1 else -1     # pinned: p1 == p2 contributes its first side only
        if o1 >= 0:
            F[blk(o1), blk(o1)] += pp_h[s, 0, :D, :D]
            rhs[blk(o1)] += pp_g[s, 0, :D]
            entries[o1].append((s, 0, o2 if o2 >= 0 else NONE, 0))
        if o2 >= 0:
            F[blk(o2), blk(o2)] += pp_h[s, 2, :D, :D]
            rhs[blk(o2)] += pp_g[s, 1, :D]
            entries[o2].append((s, 1, o1 if o1 >= 0 else NONE, 0))
        if o1 >= 0 and o2 >= 0:
            F[blk(o1), blk(o2)] += pp_h[s, 1, :D, :D]
            F[blk(o2), blk(o1)] += pp_h[s, 1, :D, :D].T
    keep = np.ones(ld, dtype=bool)
    for p in range(g.P):
        if opt[p] >= 0:
            for k in range(D):
                if g.masks[p] >> k & 1:
                    keep[opt[p] * D + k] = False
    F[~keep, :] = 0.0
    F[:, ~keep] = 0.0
    rhs[~keep] = 0.0
    # lower storage: blocks (j, i) with i < j, and the diagonal blocks with both triangles
    b = np.arange(ld) // D
    b[n_p:] = np.iinfo(np.int64).max
    F[b[:, None] < b[None, :]] = 0.0
    # the pattern: coupled active blocks, pose diagonals, tile diagonal, calibration border
    pairs = [(p1, p2) for p1, p2 in g.binary + g.imu]
    pairs += [(q[k], q[k2]) for q in g.priors for k in range(len(q)) for k2 in range(k + 1)]
    for p1, p2 in pairs:
        if opt[p1] >= 0 and opt[p2] >= 0:
            touched[blk(opt[p1]), blk(opt[p2])] = True
    for o in range(g.Pact):
        touched[blk(o), blk(o)] = True
    touched[np.arange(ld), np.arange(ld)] = True
    if g.K:
        touched[n_p:n, :n] = True
    touched |= touched.T
    nt = ld // 64
    tiles = touched.reshape(nt, 64, nt, 64).any(axis=(1, 3))
    return F, rhs, tiles, entries


def group_edges(g):
    """group pairs of the binary and inertial residuals and the prior cliques, natural order, duplicates kept"""
    G = 64 // math.gcd(g.D, 64)
    nat = g.natural_opt()
    pairs = list(g.binary) + list(g.imu)
    pairs += [(q[k], q[k2]) for q in g.priors for k in range(len(q)) for k2 in range(k)]
    out = []
    for p1, p2 in pairs:
        if p1 >= g.P or p2 >= g.P or nat[p1] < 0 or nat[p2] < 0:
            continue
        a, b = int(nat[p1]) // G, int(nat[p2]) // G
        if a != b:
            out.append(min(a, b) << 32 | max(a, b))
    return sorted(out)


def host_group_edges(hc, g):
    u32 = ctypes.c_uint32
    b1, b2 = _u32([a for a, _ in g.binary]), _u32([b for _, b in g.binary])
    i1, i2 = _u32([a for a, _ in g.imu]), _u32([b for _, b in g.imu])
    qptr, qpose = _prior_csr(g)
    cap = len(g.binary) + len(g.imu) + sum(len(q) * len(q) for q in g.priors) + 1
    out = np.zeros(cap, dtype=np.uint64)
    k = hc.ba_hostcheck_coupling_group_edges(g.D, g.P, _ptr(g.active, ctypes.c_uint8), len(b1), _ptr(b1, u32), _ptr(b2, u32),
                                             len(i1), _ptr(i1, u32), _ptr(i2, u32), len(g.priors), _ptr(qptr, u32),
                                             _ptr(qpose, u32), _ptr(out, ctypes.c_uint64), cap)
    assert k < cap
    return sorted(int(e) for e in out[:k])


# ---- the graphs ---------------------------------------------------------------------------------------------------
def _active(P, inactive):
    a = np.ones(P, dtype=np.uint8)
    a[list(inactive)] = 0
    return a


# PoseSize 6, 16 poses, 3 and 7 inactive: 14 active, opt id 10 = pose 12 holds rows 60 .. 65 (tiles 0 and 1)
D6 = Graph(
    6, _active(16, [3, 7]),
    unary=[0, 12, 3, 12, 15],                       # pose 3: a unary residual on an inactive pose
    binary=[(1, 2), (5, 4), (1, 2), (2, 1),         # opt(p1) < opt(p2); >; the same pair twice; both directions
            (6, 6),                                 # p1 == p2
            (3, 4), (4, 7), (3, 7),                 # p1 inactive; p2 inactive; both
            (12, 0), (13, 12), (12, 14), (15, 8)],  # the straddling pose as row and as column block
    imu=[(8, 9), (9, 10), (10, 11), (11, 12), (12, 13), (7, 8), (13, 13)],
    priors=[[5], [0, 12, 15], [4, 3, 9]],           # cliques of 1 and 3, one with an inactive member
    masks={12: 0x7, 0x0: 0x38, 2: 0x5, 3: 0x3F})   # on a row pose (12 over 0), on the other pose (0), on an inactive one

# PoseSize 15, 8 poses, 1 inactive: 7 active, opt id 4 = pose 5 holds rows 60 .. 74
D15 = Graph(
    15, _active(8, [1]),
    unary=[5, 1, 0],
    binary=[(5, 0), (2, 5), (5, 6), (6, 5), (1, 5), (4, 4)],
    imu=[(0, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 6), (3, 1), (3, 4)],
    priors=[[7], [5, 0, 1]],
    masks={5: 0x4003, 0: 0x0700, 6: 0x1})

# ---- graphs whose tile pattern has zeros: every decisive tile has ONE source ----------------------------------------
# PoseSize 6, 24 poses (three tiles).  Tile (2, 0) comes from the binary residual (23, 0) alone; everything else lies in
# the band that the straddling poses 10 (tiles 0 / 1) and 21 (tiles 1 / 2) mark anyway.
FAR = Graph(6, _active(24, []), unary=[23], binary=[(23, 0), (11, 10)], imu=[(21, 20)], priors=[[2], [20, 12, 13]])

# PoseSize 15, 24 active poses = 360 rows = 6 tiles (pose 24 is inactive and last, so opt id = pose id).  Pose p holds
# rows 15 p .. 15 p + 14: poses 4, 8, 12, 17, 21 straddle tiles 0/1, 1/2, 2/3, 3/4, 4/5 and their diagonal blocks mark
# the band (t + 1, t).  The ten off-band tiles:
#   (2, 0)          binary (9, 0)          neither pose straddles
#   (4, 2), (5, 2)  binary (21, 10)        the ROW pose straddles tiles 4 / 5, the column pose does not
#   (3, 1)          inertial (14, 5)
#   (5, 0), (5, 1)  inertial (23, 4)       the COLUMN pose straddles tiles 0 / 1
#   (4, 0)          prior clique [18, 1]
#   (3, 0), (4, 1), (5, 3)                 nothing: must stay 0; (24, 2) and the clique [24, 13, 14] have an inactive
#                                          member and the active pair (14, 13) lies in tile (3, 3)
TILES15 = Graph(15, _active(25, [24]), unary=[3, 24],
                binary=[(9, 0), (21, 10), (24, 2)], imu=[(14, 5), (23, 4)], priors=[[18, 1], [6], [24, 13, 14]],
                masks={21: 0x11, 10: 0x4000})
TILES15_SOURCES = {"binary": [(2, 0), (4, 2), (5, 2)], "imu": [(3, 1), (5, 0), (5, 1)], "priors": [(4, 0)]}
TILES15_EMPTY = [(3, 0), (4, 1), (5, 3)]

# Calibration border (K = 6) as the only source of its tiles.  name: (graph, tile rows of the border, tiles that only the
# border marks, tiles that must stay 0)
BORDERS = {
    # PoseSize 6, 21 poses: np = 126, border rows 126 .. 131 in tile rows 1 and 2; no pose straddles tiles 1 / 2
    "border_d6_rows_1_2": (Graph(6, _active(21, []), unary=[0], binary=[(1, 0)], K=6), [1, 2], [(2, 0), (2, 1)], []),
    # PoseSize 6, 22 poses: np = 132, border rows 132 .. 137 in tile row 2 (pose 21 straddles 1 / 2 and marks (2, 1))
    "border_d6_row_2": (Graph(6, _active(22, []), imu=[(1, 0)], K=6), [2], [(2, 0)], []),
    # PoseSize 9, 21 poses: np = 189, border rows 189 .. 194 in tile rows 2 and 3; poses 7 and 14 straddle 0/1 and 1/2,
    # so (2, 0) is the FIRST border tile row's alone and (3, 0) .. (3, 2) the last one's
    "border_d9_rows_2_3": (Graph(9, _active(21, []), unary=[20], K=6), [2, 3], [(2, 0), (3, 0), (3, 1), (3, 2)], []),
    # PoseSize 9, 22 poses: np = 198, border rows 198 .. 203 in tile row 3 alone (pose 21 straddles 2 / 3 and marks
    # (3, 2)): (2, 0) stays 0
    "border_d9_row_3": (Graph(9, _active(22, []), binary=[(2, 1)], K=6), [3], [(3, 0), (3, 1)], [(2, 0)]),
}

# 70 poses of PoseSize 6 (pose 40 inactive) = 414 rows = 7 tiles, three pose groups of 32
GROUPS3 = Graph(6, _active(70, [40]), unary=[69], binary=[(0, 69), (69, 0), (0, 40), (1, 2), (33, 31)],
                imu=[(31, 32), (64, 65)], priors=[[0, 35, 69], [40, 1, 68]])

CASES = {
    "d6_straddle": D6,
    "d15_straddle": D15,
    "d6_reversed_order": D6.with_(perm=np.arange(14)[::-1]),
    "d6_shuffled_order": D6.with_(perm=np.random.default_rng(5).permutation(14)),
    "d15_shuffled_order": D15.with_(perm=[3, 6, 0, 5, 1, 4, 2]),
    "no_unary": D6.with_(unary=[]),
    "no_binary": D6.with_(binary=[]),
    "no_imu": D6.with_(imu=[]),
    "only_unary": D6.with_(binary=[], imu=[], priors=[]),
    "no_residuals": D6.with_(unary=[], binary=[], imu=[], priors=[]),
    "no_active_pose": D6.with_(active=np.zeros(16, dtype=np.uint8), priors=[]),
    "far_tiles": FAR,
    "tiles_d15": TILES15,
    "tiles_d15_no_binary": TILES15.with_(binary=[]),
    "tiles_d15_no_imu": TILES15.with_(imu=[]),
    "tiles_d15_no_priors": TILES15.with_(priors=[]),
    "tiles_d15_shuffled_order": TILES15.with_(perm=np.random.default_rng(7).permutation(24)),
    "three_groups": GROUPS3,
    # K = 6: np = 60 (border rows 60 .. 65: two tile rows) and np = 66 (rows 66 .. 71: one)
    "border_two_tile_rows": Graph(6, _active(12, [4, 9]), unary=[0], binary=[(11, 0), (3, 4)], imu=[(1, 2)], K=6),
    "border_one_tile_row": Graph(6, _active(12, [4]), unary=[0], binary=[(11, 0), (3, 4)], imu=[(1, 2)], K=6),
    "border_only": Graph(6, _active(11, []), K=6),
}
CASES.update({name: b[0] for name, b in BORDERS.items()})


def pattern(g):
    return brute_force(g, *random_blocks(g, 0))[2]


@pytest.mark.parametrize("name", list(CASES))
def test_lists_reproduce_the_brute_force_sum(hc, name):
    g = CASES[name]
    pp_h, pp_g = random_blocks(g, 100 + list(CASES).index(name))
    rc, msg, out = host_lists(hc, g, pp_h, pp_g)
    assert (rc, msg) == (0, "")
    n, ld, nt = out["n"], out["ld"], out["nt"]
    S_ref, rhs_ref, tiles_ref, entries = brute_force(g, pp_h, pp_g)
    n_ent = sum(len(e) for e in entries)
    assert list(out["counts"]) == [g.Pact, n, ld, n_ent, len(g.slots)]
    # the lists themselves: per pose its entries in slot order
    assert out["pp_ptr"][0] == 0 and list(np.diff(out["pp_ptr"].astype(np.int64))) == [len(e) for e in entries]
    assert [tuple(int(x) for x in r) for r in out["pp_ent"][:n_ent]] == [t for e in entries for t in e]
    # S and the right-hand side, exactly (module docstring); tril as a statement of its own
    S = out["S"]
    assert np.array_equal(np.tril(S), np.tril(S_ref))
    assert np.array_equal(S, S_ref)
    assert np.array_equal(out["rhs"], rhs_ref)
    assert not S[n:, :].any() and not S[:, n:].any()
    # the tile pattern
    tiles = out["tile_nz"]
    assert set(np.unique(tiles)) <= {0, 1}
    assert np.array_equal(tiles, tiles.T)
    assert np.array_equal(tiles.astype(bool), tiles_ref)
    nz_tiles = (S != 0).reshape(nt, 64, nt, 64).any(axis=(1, 3))
    assert not (nz_tiles & ~tiles.astype(bool)).any()


def _lower(tiles):
    return {(int(r), int(c)) for r, c in zip(*np.nonzero(tiles)) if c <= r}


def test_cases_cover_what_they_claim():
    opt6, opt15 = D6.pose_opt(), D15.pose_opt()
    assert D6.Pact >= 12 and opt6[12] == 10 and D15.Pact >= 6 and opt15[5] == 4
    assert opt6[5] > opt6[4] and opt6[1] < opt6[2] and D6.binary.count((1, 2)) == 2 and (2, 1) in D6.binary
    _, _, tiles, entries = brute_force(D6, *random_blocks(D6, 0))
    slot = {pair: len(D6.unary) + i for i, pair in enumerate(D6.binary)}
    assert tiles[1, 0]
    assert [e for e in entries[opt6[6]] if e[0] == slot[(6, 6)]] == [(slot[(6, 6)], 0, NONE, 0)]   # p1 == p2: one entry
    assert not any(e[0] == slot[(3, 7)] for es in entries for e in es)                             # both inactive: none
    assert sum(e[0] == slot[(3, 4)] for es in entries for e in es) == 1                            # one inactive: one
    two, one = CASES["border_two_tile_rows"], CASES["border_one_tile_row"]
    assert two.Pact * 6 == 60 and one.Pact * 6 == 66


def test_tile_cases_have_zeros_and_single_sources():
    """The expected patterns themselves (the brute force, no library): each decisive tile is there, goes away with its
    one source and with nothing else, and the tiles named empty are empty."""
    # FAR: (2, 0) is the binary residual (23, 0)'s alone
    far = _lower(pattern(FAR))
    assert far == {(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (2, 0)}
    assert _lower(pattern(FAR.with_(binary=[(11, 10)]))) == far - {(2, 0)}
    assert _lower(pattern(FAR.with_(imu=[], priors=[], unary=[]))) == far
    # TILES15: band + seven off-band tiles, three empty; each kind owns exactly its tiles
    band = {(t, t) for t in range(6)} | {(t + 1, t) for t in range(5)}
    full = _lower(pattern(TILES15))
    owned = {k: set(v) for k, v in TILES15_SOURCES.items()}
    assert full == band | owned["binary"] | owned["imu"] | owned["priors"] and len(full) == len(band) + 7
    assert not full & set(TILES15_EMPTY) and len(set(TILES15_EMPTY)) == 3
    for kind, mine in owned.items():
        assert _lower(pattern(TILES15.with_(**{kind: []}))) == full - mine
    assert _lower(pattern(TILES15.with_(binary=[(9, 0), (24, 2)]))) == full - {(4, 2), (5, 2)}     # the straddling row pose
    assert _lower(pattern(TILES15.with_(imu=[(14, 5)]))) == full - {(5, 0), (5, 1)}                # the straddling column pose
    assert _lower(pattern(TILES15.with_(binary=[], imu=[], priors=[]))) == band
    # the pattern under the shuffled order is another one, and has zeros too
    shuffled = _lower(pattern(CASES["tiles_d15_shuffled_order"]))
    assert shuffled != full and len(shuffled) < 21
    # borders: the tile rows, the tiles only the border marks, the tiles nothing marks
    for name, (g, rows, only_border, empty) in BORDERS.items():
        n_p, n = g.Pact * g.D, g.Pact * g.D + g.K
        assert list(range(n_p // 64, (n - 1) // 64 + 1)) == rows, name
        with_border, without = _lower(pattern(g)), _lower(pattern(g.with_(K=0)))
        nt = (n + 63) // 64
        without = {t for t in without if t[0] < nt}
        assert with_border - without == set(only_border) | ({(nt - 1, nt - 1)} if (n_p + 63) // 64 < nt else set()), name
        assert not with_border & set(empty), name
        assert all(r in rows for r, _ in only_border), name
    # one graph in which BOTH tile rows of a two-row border own a tile
    assert {r for r, _ in BORDERS["border_d9_rows_2_3"][2]} == {2, 3}
    # the multi-group graph has empty tiles as well
    assert len(_lower(pattern(GROUPS3))) < 7 * 8 // 2


@pytest.mark.parametrize("where", ["unary", "binary_p1", "binary_p2", "imu_p1", "imu_p2"])
def test_unknown_pose_is_refused_with_the_engines_message(hc, where):
    bad = D6.P
    g = {"unary": D6.with_(unary=D6.unary + [bad]),
         "binary_p1": D6.with_(binary=D6.binary + [(bad, 1)]),
         "binary_p2": D6.with_(binary=D6.binary + [(1, bad + 5)]),
         "imu_p1": D6.with_(imu=[(bad, 1)] + D6.imu),
         "imu_p2": D6.with_(imu=D6.imu + [(1, NONE - 1)])}[where]
    rc, msg, _ = host_lists(hc, g, *random_blocks(g, 1))
    assert (rc, msg) == (1, UNKNOWN_POSE)


# graphs with more than one pose group (32 poses of PoseSize 6, 64 of PoseSize 15 to a group)
MULTI_GROUP = {
    "three_groups": GROUPS3,
    "three_groups_unknown_pose": GROUPS3.with_(binary=GROUPS3.binary + [(0, 700)]),   # ignored by the ordering's filter
    "two_groups_d6": Graph(6, _active(40, [5, 33]), binary=[(0, 39), (39, 0), (34, 2), (33, 1), (36, 37)], imu=[(32, 35), (31, 34)],
                           priors=[[39], [1, 38, 5], [2, 3, 4]]),
    "two_groups_d15": Graph(15, _active(70, []), binary=[(0, 69), (63, 64), (10, 20)], imu=[(64, 65)], priors=[[69, 1, 68]]),
}


@pytest.mark.parametrize("name", list(MULTI_GROUP))
def test_coupling_enumeration_gives_the_orderings_group_edges(hc, name):
    g = MULTI_GROUP[name]
    ref = group_edges(g)
    assert len(ref) >= 3 and len(set(ref)) < len(ref)     # edges, and duplicates among them
    assert host_group_edges(hc, g) == ref


def test_group_edges_of_the_three_group_graph():
    # 32 poses to a group; natural ids: pose 40 is inactive, so poses 65 .. 69 are group 2
    ref = group_edges(MULTI_GROUP["three_groups_unknown_pose"])
    assert [ref.count(e) for e in (0 << 32 | 1, 0 << 32 | 2, 1 << 32 | 2)] == [3, 4, 2] and len(ref) == 9
    assert ref == group_edges(GROUPS3)
