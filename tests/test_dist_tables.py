"""The derived tables of the distributed solve (ba_amd/csrc/dist_plan.h: owned block pairs, square rows, the rows of
the dense reduce-scatter, the rectangles of the sparse exchange of S, the assembly's tiles, the staging capacities and
the flop count of a bulk update) on the CPU, through ba_hostcheck_dist_tables.

Everything is compared with brute-force restatements written from the header's comments: the owner of a block is
tbl[class of its row][class of its column], and each table is a filter over all tiles.  The one that matters is the
symmetry of the sparse exchange: what rank a sends to rank b must be, rectangle for rectangle, what b expects from a —
on a machine a mismatch is a hang or a wrong sum, and only these tests can see it without eight GPUs."""
import ctypes
import math

import numpy as np
import pytest

from helpers import hostcheck_lib

NB = 64
LAYOUTS = [(1, "single"), (2, "tri"), (3, "grid"), (4, "grid"), (8, "tri"), (3, "col"), (3, "row")]
NBLKS = [5, 8, 9, 13]          # a ragged last panel, an exact multiple, odd counts
WIDTHS = [2, 3, 4]
REFUSAL = b"sparse exchange of S: more than 2^32 doubles to one side (use BA_HIP_DENSE_SCATTER=1)"
grid = pytest.mark.parametrize("nranks,layout", LAYOUTS, ids=["%d_%s" % (n, l) for n, l in LAYOUTS])
sizes = pytest.mark.parametrize("nblk", NBLKS)


# ---- the tap -------------------------------------------------------------------------------------------------------
def tap(op, nblk, G, N, rank, layout, nzL=None, nz2=None, bits=None, arg=(), want_msg=False):
    hc = hostcheck_lib()
    f = hc.ba_hostcheck_dist_tables
    f.restype = ctypes.c_int64
    u8, i64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, u8, u8, ctypes.POINTER(ctypes.c_uint64), i64,
                  i64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32]
    hdr = (ctypes.c_uint32 * 4)(nblk, G, N, rank)
    keep = [np.ascontiguousarray(x, dtype=np.uint8) if x is not None else None for x in (nzL, nz2)]
    ptr = [x.ctypes.data_as(u8) if x is not None else None for x in keep]
    b = np.ascontiguousarray(bits, dtype=np.uint64) if bits is not None else None
    a = np.ascontiguousarray(list(arg) + [0] * 4, dtype=np.int64)
    out = np.zeros(8 * nblk * nblk * max(N, 1) + 4096, dtype=np.int64)
    msg = ctypes.create_string_buffer(160)
    n = f(op, hdr, None if layout == "single" else layout.encode(), ptr[0], ptr[1],
          b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if b is not None else None, a.ctypes.data_as(i64),
          out.ctypes.data_as(i64), out.size, msg, 160)
    assert n >= 0, (op, n)
    return (out[:n].copy(), msg.value) if want_msg else out[:n].copy()


def test_unknown_op_and_missing_layout():
    hc = hostcheck_lib()
    hc.ba_hostcheck_dist_tables.restype = ctypes.c_int64
    with pytest.raises(AssertionError):
        tap(99, 5, 2, 2, 0, "tri")
    with pytest.raises(AssertionError):
        tap(1, 5, 2, 3, 0, "tri")     # tri exists for 2, 8, 18 ranks only


# ---- restatement of the ownership map (dist_plan.h, the header comment) ------------------------------------------------
def own_table(N, layout):
    """classes T and tbl[a][b]"""
    if N == 1:
        return 1, [[0]]
    if layout == "tri":
        T = next(t for t in range(2, 17, 2) if t * t // 2 == N)
        tbl = [[None] * T for _ in range(T)]
        r = 0
        for a in range(T):                      # the "cross" ranks: one unordered class pair each
            for b in range(a + 1, T):
                tbl[a][b] = tbl[b][a] = r
                r += 1
        for k in range(T // 2):                 # the "diagonal" ranks: the blocks (a, a) of two classes
            tbl[2 * k][2 * k] = tbl[2 * k + 1][2 * k + 1] = r + k
        return T, tbl
    if layout == "grid":
        pr = max(d for d in range(1, N + 1) if d * d <= N and N % d == 0)
        pc = N // pr
        T = pr * pc // math.gcd(pr, pc)
        return T, [[(a % pr) * pc + b % pc for b in range(T)] for a in range(T)]
    return N, [[b if layout == "col" else a for b in range(N)] for a in range(N)]


class Plan:
    def __init__(self, nblk, G, N, layout):
        self.nblk, self.G, self.N, self.layout = nblk, G, N, layout
        self.T, self.tbl = own_table(N, layout)
        self.nb = (nblk + G - 1) // G
        self.panels = [(J * G, min(J * G + G, nblk)) for J in range(self.nb)]

    def owner(self, i, c):
        """of tile (i, c), i >= c; i == nblk is the rhs row, which rides with the diagonal block of its column"""
        cc = (c // self.G) % self.T
        rc = cc if i == self.nblk else (i // self.G) % self.T
        return self.tbl[rc][cc]

    def tap(self, op, rank=0, **kw):
        return tap(op, self.nblk, self.G, self.N, rank, self.layout, **kw)


def test_own_table_is_the_headers():
    for N, layout in LAYOUTS:
        p = Plan(8, 2, N, layout)
        t = p.tap(7)
        nb, T = int(t[0]), int(t[1])
        assert (nb, T) == (p.nb, p.T)
        assert t[3:3 + T * T].reshape(T, T).tolist() == p.tbl
        assert sorted(set(sum(p.tbl, []))) == list(range(N))      # every rank owns something


# ---- patterns ----------------------------------------------------------------------------------------------------------
def close_factor(nz):
    hc = hostcheck_lib()
    hc.ba_hostcheck_tile_factor.restype = ctypes.c_uint64
    out = np.ascontiguousarray(nz, dtype=np.uint8).copy()
    hc.ba_hostcheck_tile_factor(ctypes.c_uint32(out.shape[0]), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return out


def factor_patterns(nblk):
    """name -> (S pattern, factor pattern): lower, with the diagonal; the factor pattern is closed under elimination"""
    i, k = np.indices((nblk, nblk))
    low = i >= k
    pats = {"dense": low, "band2": low & (i - k <= 2), "arrow": (i == k) | (low & (i == nblk - 1))}
    for seed in (3, 11):
        rng = np.random.default_rng(1000 * nblk + seed)
        pats["random%d" % seed] = (i == k) | (low & (rng.random((nblk, nblk)) < 0.25))
    out = {}
    for name, s in pats.items():
        s = s.astype(np.uint8)
        f = close_factor(s)
        assert np.all(f >= s) and np.all(np.triu(f, 1) == 0)
        if not name.startswith("random"):
            assert np.array_equal(f, s)
        out[name] = (s, f)
    return out


def local_patterns(S, N, seed):
    """kind -> one pattern per rank; their union is S, and like a shard's every one holds the diagonal"""
    nblk = S.shape[0]
    i, k = np.indices(S.shape)
    diag = (i == k)
    rng = np.random.default_rng(seed)
    mask = rng.integers(1, 2 ** N, size=S.shape) if N < 63 else None       # a non-empty set of ranks per tile
    kinds = {"bands": [((S != 0) & ((i * N // nblk == r) | diag)).astype(np.uint8) for r in range(N)],
             "everything": [S.copy() for _ in range(N)],
             "random": [((S != 0) & (((mask >> r) & 1 == 1) | diag)).astype(np.uint8) for r in range(N)]}
    for pats in kinds.values():
        assert np.array_equal(np.maximum.reduce(pats), S)
    return kinds


def pack_bits(pats):
    nblk = pats[0].shape[0]
    words = (nblk * nblk + 63) // 64
    out = np.zeros((len(pats), words), dtype=np.uint64)
    for r, p in enumerate(pats):
        for b in np.flatnonzero(np.tril(p).reshape(-1)):
            out[r, b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return out


def has_tile(pat, i, c0, c1):
    return any(pat[i, kb] for kb in range(c0, min(c1, i + 1)))


class Rects:
    """the result of dist_sparse_rects for one rank"""

    def __init__(self, t, N):
        self.refused, ns, nr = int(t[0]), int(t[1]), int(t[2])
        o = 3
        self.send_first, self.recv_first, self.send_off, self.recv_off = (t[o + j * (N + 1):o + (j + 1) * (N + 1)].tolist() for j in range(4))
        o += 4 * (N + 1)
        self.send = t[o:o + 4 * ns].reshape(ns, 4).tolist()
        self.recv = t[o + 4 * ns:o + 4 * (ns + nr)].reshape(nr, 4).tolist()
        assert len(t) == o + 4 * (ns + nr)

    def to(self, peer):
        return self.send[self.send_first[peer]:self.send_first[peer + 1]]

    def frm(self, peer):
        return self.recv[self.recv_first[peer]:self.recv_first[peer + 1]]


def all_rects(p, bits, limit=-1):
    return [Rects(p.tap(3, rank=r, bits=bits, arg=[limit]), p.N) for r in range(p.N)]


# ---- the sparse exchange of S -------------------------------------------------------------------------------------------
@grid
@sizes
def test_exchange_symmetry(nranks, layout, nblk):
    N = nranks
    for G in WIDTHS:
        p = Plan(nblk, G, N, layout)
        for pname, (S, _) in factor_patterns(nblk).items():
            for kind, pats in local_patterns(S, N, 7 * nblk + G).items():
                rk = all_rects(p, pack_bits(pats))
                for a in range(N):
                    ra = rk[a]
                    assert not ra.refused
                    assert ra.to(a) == [] and ra.frm(a) == []                  # nothing to oneself
                    for lst, first, off in ((ra.send, ra.send_first, ra.send_off), (ra.recv, ra.recv_first, ra.recv_off)):
                        run = 0
                        for row, col, width, o in lst:                          # offsets: running sums of 64 * width
                            assert o == run
                            run += NB * width
                        assert off[N] == run and first[0] == 0 and first[N] == len(lst)
                        for peer in range(N):
                            assert off[peer] == sum(NB * w for _, _, w, _ in lst[:first[peer]])
                    for b in range(N):
                        if a == b:
                            continue
                        sent = [x[:3] for x in ra.to(b)]
                        assert sent == [x[:3] for x in rk[b].frm(a)], (G, pname, kind, a, b)
                        assert ra.send_off[b + 1] - ra.send_off[b] == rk[b].recv_off[a + 1] - rk[b].recv_off[a]
                        # the rule: a rectangle (row tile, panel) goes to its owner iff the sender's pattern has a tile in it;
                        # by panel, then by row tile — and so each exactly once
                        want = [[i, c0 * NB, (c1 - c0) * NB] for c0, c1 in p.panels for i in range(c0, nblk)
                                if p.owner(i, c0) == b and has_tile(pats[a], i, c0, c1)]
                        assert sent == want, (G, pname, kind, a, b)


@grid
@sizes
def test_exchange_overflow_refusal(nranks, layout, nblk):
    N = nranks
    G = 3
    p = Plan(nblk, G, N, layout)
    S, _ = factor_patterns(nblk)["band2"]
    bits = pack_bits(local_patterns(S, N, 5)["everything"])
    for r in range(N):
        t, msg = p.tap(3, rank=r, bits=bits, arg=[-1], want_msg=True)
        rr = Rects(t, N)
        assert not rr.refused and msg == b""                       # the default limit: never on this grid
        most = max(rr.send_off[N], rr.recv_off[N])
        t, msg = p.tap(3, rank=r, bits=bits, arg=[most], want_msg=True)
        assert not Rects(t, N).refused and msg == b""              # exactly at the limit
        if most:
            for limit in (most - 1, NB * NB - 1, 0):
                t, msg = p.tap(3, rank=r, bits=bits, arg=[limit], want_msg=True)
                assert Rects(t, N).refused == 1 and msg == REFUSAL
        else:
            assert N == 1


# ---- the tiles the assembly writes --------------------------------------------------------------------------------------
@grid
@sizes
def test_assembly_need(nranks, layout, nblk):
    N = nranks
    for G in WIDTHS:
        p = Plan(nblk, G, N, layout)
        for pname, (S, F) in factor_patterns(nblk).items():
            for kind, pats in local_patterns(S, N, 13 * nblk + G).items():
                rk = all_rects(p, pack_bits(pats))
                for r in range(N):
                    need = p.tap(4, rank=r, nzL=F, nz2=pats[r]).reshape(nblk, nblk)
                    want = np.zeros((nblk, nblk), dtype=np.int64)
                    for c0, c1 in p.panels:
                        for i in range(c0, nblk):
                            if p.owner(i, c0) == r or has_tile(pats[r], i, c0, c1):      # owned, or sent
                                for kb in range(c0, min(c1, i + 1)):
                                    want[i, kb] = F[i, kb]
                    assert np.array_equal(need, want), (G, pname, kind, r)
                    for row, col, width, _ in rk[r].send:                              # a rectangle travels whole
                        c0, c1 = col // NB, (col + width) // NB
                        for kb in range(c0, min(c1, row + 1)):
                            assert need[row, kb] == F[row, kb]


# ---- tables of the plan alone -------------------------------------------------------------------------------------------
@grid
@sizes
def test_owned_pairs(nranks, layout, nblk):
    N = nranks
    for G in WIDTHS:
        p = Plan(nblk, G, N, layout)
        seen = []
        for r in range(N):
            t = p.tap(0, rank=r)
            npairs, first = int(t[0]), t[1:p.nb + 2].tolist()
            pairs = t[p.nb + 2:].reshape(npairs, 2).tolist()
            assert first == sorted(first) and len(first) == p.nb + 1 and first[p.nb] == npairs
            mine = [[bi, bc] for bc in range(p.nb) for bi in range(bc, p.nb) if p.tbl[bi % p.T][bc % p.T] == r]
            assert pairs == mine
            for J in range(p.nb + 1):
                assert pairs[first[J]:] == [q for q in mine if q[1] >= J + 2]
            seen += [tuple(q) for q in pairs]
        assert sorted(seen) == [(bi, bc) for bi in range(p.nb) for bc in range(bi + 1)]   # a partition of the blocks


@grid
@sizes
def test_square_rows(nranks, layout, nblk):
    for G in WIDTHS:
        p = Plan(nblk, G, nranks, layout)
        want = []
        for c0, c1 in p.panels:
            want += list(range(c0, c1)) + [nblk]
        for r in range(nranks):
            assert p.tap(1, rank=r).tolist() == want


@grid
@sizes
def test_dense_scatter_rows(nranks, layout, nblk):
    N = nranks
    for G in WIDTHS:
        p = Plan(nblk, G, N, layout)
        pats = [(None, None)] + list(factor_patterns(nblk).values())
        for S, F in pats:
            t = p.tap(2, nzL=F, nz2=S)
            chunk, nrows = int(t[0]), int(t[1])
            n = p.nb * N
            off, coff, rows = t[2:n + 3].tolist(), t[n + 3:2 * n + 3].tolist(), t[2 * n + 3:].tolist()
            assert len(rows) == nrows == off[n] and off[0] == 0
            used = [[] for _ in range(N)]
            for J, (c0, c1) in enumerate(p.panels):
                for r in range(N):
                    k = J * N + r
                    want = [i for i in range(c0, nblk) if p.owner(i, c0) == r and (S is None or has_tile(S, i, c0, c1))]
                    assert rows[off[k]:off[k + 1]] == want
                    used[r].append((coff[k], coff[k] + len(want) * NB * (c1 - c0) * NB))
            assert chunk % 64 == 0
            for r in range(N):
                end = 0
                for lo, hi in used[r]:          # panels in order, back to back: no overlap
                    assert lo == end
                    end = hi
                assert end <= chunk
            assert chunk - 64 < max(u[-1][1] for u in used)


@grid
@sizes
def test_staging_caps(nranks, layout, nblk):
    N = nranks
    for G in WIDTHS:
        p = Plan(nblk, G, N, layout)
        for S, F in [(None, None)] + list(factor_patterns(nblk).values()):
            t = p.tap(7, nzL=F)
            nb, T, nmsgs = (int(x) for x in t[:3])
            o = 3 + T * T
            panels = t[o:o + 3 * nb].reshape(nb, 3).tolist()
            assert [q[:2] for q in panels] == [list(q) for q in p.panels]
            assert [q[2] for q in panels] == [p.owner(c0, c0) for c0, _ in p.panels]
            o += 3 * nb
            msgs = []
            for _ in range(nmsgs):
                panel, src, urgent, ntiles, ndst = (int(x) for x in t[o:o + 5])
                dst = t[o + 5 + ntiles:o + 5 + ntiles + ndst].tolist()
                msgs.append((panel, src, urgent, ntiles, dst))
                o += 5 + ntiles + ndst
            assert o == len(t)
            for r in range(N):
                caps = {(u, d): 1 for u in (0, 1) for d in "sr"}
                for J, (c0, c1) in enumerate(p.panels):
                    tot = {k: 0 for k in caps}
                    for panel, src, urgent, ntiles, dst in msgs:
                        if panel != J:
                            continue
                        cnt = ntiles * NB * (c1 - c0) * NB
                        if src == r:
                            tot[(urgent, "s")] += cnt
                        if r in dst:
                            tot[(urgent, "r")] += cnt
                    caps = {k: max(caps[k], tot[k]) for k in caps}
                assert p.tap(5, rank=r, nzL=F).tolist() == [caps[(1, "s")], caps[(1, "r")], caps[(0, "s")], caps[(0, "r")]]


@grid
@sizes
def test_bulk_update_tile_products(nranks, layout, nblk):
    """summed over the ranks: the single-GPU count, sum over the panel's columns of m (m + 1) / 2 + m"""
    N = nranks
    for G in WIDTHS:
        p = Plan(nblk, G, N, layout)
        for S, F in [(None, None)] + list(factor_patterns(nblk).values()):
            for c0, c1 in p.panels:
                for first in sorted({min(c1 + G, nblk), c1}):
                    arg = [first, c0, c1]
                    single = int(p.tap(6, nzL=F, arg=arg + [1])[0])
                    ms = [nblk - first if F is None else int(F[first:, kb].sum()) for kb in range(c0, c1)]
                    assert single == sum(m * (m + 1) // 2 + m for m in ms)
                    assert sum(int(p.tap(6, rank=r, nzL=F, arg=arg + [0])[0]) for r in range(N)) == single
