"""Pose ordering of the reduced camera solve (ba_amd/csrc/ordering.h), checked on the CPU through
libba_hostcheck.so: the chosen permutation keeps tile-aligned groups whole and the tail last, the shared
symbolic tile elimination matches a brute-force LDL^T fill, and AUTO never needs more tile products than
natural order (on a multi-lap route far fewer)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u32p = ctypes.POINTER(ctypes.c_uint32)
u8p = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_tile_factor.restype = ctypes.c_uint64
    lib.ba_hostcheck_group_order_products.restype = ctypes.c_uint64
    return lib


def group_size(D):
    return 64 // np.gcd(D, 64)


def csr(ng, pairs):
    """Symmetric CSR of group pairs (self loops dropped)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    both = np.unique(np.concatenate([pairs, pairs[:, ::-1]]), axis=0) if len(pairs) else np.zeros((0, 2), np.int64)
    ptr = np.zeros(ng + 1, dtype=np.uint32)
    np.add.at(ptr, both[:, 0] + 1, 1)
    return np.cumsum(ptr).astype(np.uint32), np.ascontiguousarray(both[:, 1], dtype=np.uint32)


def pose_pairs_to_groups(pairs, G):
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2) // G


def order(hc, Pact, D, K, ptr, adj):
    perm = np.zeros(max(Pact, 1), dtype=np.uint32)
    cand, g = ctypes.c_int(), ctypes.c_uint32()
    prod = np.zeros(4, dtype=np.uint64)
    Pact, D, K = int(Pact), int(D), int(K)
    hc.ba_hostcheck_pose_ordering(Pact, D, K, ptr.ctypes.data_as(u32p), adj.ctypes.data_as(u32p),
                                  perm.ctypes.data_as(u32p), ctypes.byref(cand), ctypes.byref(g),
                                  prod.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return perm[:Pact], cand.value, g.value, prod


def check_perm(perm, Pact, G):
    assert sorted(perm.tolist()) == list(range(Pact))
    nfull = Pact // G
    for g in range(nfull):
        blk = perm[g * G:(g + 1) * G].astype(np.int64)
        assert blk[0] % G == 0, "group start off the tile grid"
        assert np.array_equal(blk, blk[0] + np.arange(G)), "group split or reordered"
    # the partial group stays last, in order
    assert np.array_equal(perm[nfull * G:], np.arange(nfull * G, Pact))


def ring_pairs(P, w, laps=1, revisit=0.0, closures=0, open_path=False, rng=None):
    """Pose pairs of a route: neighbours within w along the path (a ring unless open_path), `closures`
    random long-range pairs, and for multi-lap routes pose i coupled to i + P/laps with probability revisit."""
    rng = rng or np.random.default_rng(0)
    i = np.arange(P)
    out = []
    for d in range(1, w + 1):
        j = i + d
        if open_path:
            out.append(np.stack([i[j < P], j[j < P]], 1))
        else:
            out.append(np.stack([i, j % P], 1))
    M = P // laps
    if laps > 1:
        for k in range(1, laps):
            sel = (rng.random(P) < revisit) & (i + k * M < P)
            for d in range(-2, 3):
                j = np.clip(i[sel] + k * M + d, 0, P - 1)
                out.append(np.stack([i[sel], j], 1))
    if closures:
        a = rng.integers(0, P, closures)
        b = rng.integers(0, P, closures)
        out.append(np.stack([a, b], 1))
    return np.concatenate(out)


@pytest.mark.parametrize("D", [6, 9, 15])
@pytest.mark.parametrize("K", [0, 6])
def test_permutation_valid_aligned_deterministic(hc, D, K):
    G = group_size(D)
    assert G == {6: 32, 9: 64, 15: 64}[D]
    rng = np.random.default_rng(D * 7 + K)
    for Pact in (1, G - 3, G, 3 * G + 5, 12 * G, 17 * G + 1):
        pairs = ring_pairs(Pact, 3, closures=Pact // 20 + 1, rng=rng) if Pact > 1 else np.zeros((0, 2), np.int64)
        ng = (Pact + G - 1) // G
        ptr, adj = csr(ng, pose_pairs_to_groups(pairs, G))
        a = order(hc, Pact, D, K, ptr, adj)
        b = order(hc, Pact, D, K, ptr, adj)
        check_perm(a[0], Pact, G)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], "not deterministic"
        assert a[2] == G
        if Pact < 2 * G:
            assert np.array_equal(a[0], np.arange(Pact))


def test_disconnected_components(hc):
    D, G = 6, 32
    Pact = 40 * G + 7
    # four separate rings of groups, interleaved in pose id
    pairs = []
    for g in range(41):
        for h in range(g + 4, 41, 4):
            if h - g <= 8:
                pairs.append((g * G, h * G))
    ptr, adj = csr(41, pose_pairs_to_groups(pairs, G))
    perm, cand, _, prod = order(hc, Pact, D, 0, ptr, adj)
    check_perm(perm, Pact, G)
    assert prod[cand] <= prod[0]
    # an edgeless graph is already optimal: natural order kept (ties go to natural)
    ptr0, adj0 = csr(41, np.zeros((0, 2)))
    perm0, cand0, _, _ = order(hc, Pact, D, 0, ptr0, adj0)
    assert cand0 == 0 and np.array_equal(perm0, np.arange(Pact))


def brute_fill(nz):
    """Symbolic LDL^T on a dense boolean pattern: L(i,j) != 0 iff S(i,j) or some k < j has L(i,k), L(j,k)."""
    n = nz.shape[0]
    a = (nz | nz.T).astype(bool)
    L = np.zeros_like(a)
    for j in range(n):
        col = a[j:, j].copy()
        for k in range(j):
            if L[j, k]:
                col |= L[j:, k]
        L[j:, j] = col
    return np.tril(L)


def brute_products(L):
    n = L.shape[0]
    tot = 0
    for k in range(n):
        m = int(L[k + 1:, k].sum())
        tot += m * (m + 1) // 2 + (m + 1) // 2 + m + 1
    return tot


def test_tile_factor_matches_brute_force(hc):
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(1, 90))
        nz = rng.random((n, n)) < rng.choice([0.02, 0.05, 0.15])
        nz = (nz | nz.T) | np.eye(n, dtype=bool)
        buf = np.ascontiguousarray(nz.astype(np.uint8))
        prod = hc.ba_hostcheck_tile_factor(n, buf.ctypes.data_as(u8p))
        L = brute_fill(nz)
        assert np.array_equal(buf.astype(bool), L), trial
        assert prod == brute_products(L)


def test_tile_factor_gives_todays_count_on_config3_pattern(hc):
    """The recorded configs[3] factor pattern is a fixed point of the shared elimination (the fill of a
    factor pattern is itself), and the products it counts are the statistic's formula."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "config3_factor_tile_pattern.npz"))
    n = int(z["nblk"])
    L = np.ascontiguousarray(np.unpackbits(z["bits"])[:n * n].reshape(n, n))
    sym = np.ascontiguousarray(np.maximum(L, L.T))
    prod = hc.ba_hostcheck_tile_factor(n, sym.ctypes.data_as(u8p))
    assert np.array_equal(sym, np.tril(L))
    assert prod == brute_products(np.tril(L).astype(bool))


def test_group_model_natural_is_identity_order(hc):
    D, G, Pact = 6, 32, 20 * 32 + 11
    pairs = ring_pairs(Pact, 4, closures=6, rng=np.random.default_rng(1))
    ng = (Pact + G - 1) // G
    ptr, adj = csr(ng, pose_pairs_to_groups(pairs, G))
    ident = np.arange(ng, dtype=np.uint32)
    p_nat = hc.ba_hostcheck_group_order_products(Pact, D, 6, ptr.ctypes.data_as(u32p), adj.ctypes.data_as(u32p),
                                                 ident.ctypes.data_as(u32p))
    _, _, _, prod = order(hc, Pact, D, 6, ptr, adj)
    assert prod[0] == p_nat
    # the same count by brute force on the expanded tile pattern
    tpg = G * D // 64
    n = Pact * D + 6
    nt = (n + 63) // 64
    nz = np.zeros((nt, nt), dtype=bool)
    tail0 = (Pact // G) * tpg

    def tiles(g):
        return range(g * tpg, (g + 1) * tpg) if g < Pact // G else range(tail0, (Pact * D + 63) // 64)
    for g in range(ng):
        for a in tiles(g):
            for b in tiles(g):
                nz[a, b] = True
            for e in adj[ptr[g]:ptr[g + 1]]:
                for b in tiles(int(e)):
                    nz[a, b] = nz[b, a] = True
    nz[(Pact * D) // 64:, :] = True
    nz[:, (Pact * D) // 64:] = True
    nz |= np.eye(nt, dtype=bool)
    assert p_nat == brute_products(brute_fill(nz))


def test_auto_never_worse_than_natural(hc):
    rng = np.random.default_rng(11)
    kinds = []
    for t in range(50):
        D = [6, 9, 15][t % 3]
        G = group_size(D)
        P = int(rng.integers(4, 60)) * G + int(rng.integers(0, G))
        kind = t % 5
        if kind == 0:
            pairs = ring_pairs(P, int(rng.integers(2, 40)), rng=rng)
        elif kind == 1:
            pairs = ring_pairs(P, int(rng.integers(2, 30)), closures=int(rng.integers(1, 40)), open_path=True, rng=rng)
        elif kind == 2:
            pairs = ring_pairs(P, int(rng.integers(2, 30)), closures=int(rng.integers(1, 40)), rng=rng)
        else:
            pairs = ring_pairs(P, int(rng.integers(2, 30)), laps=int(rng.integers(2, 5)), revisit=rng.random() * 0.3,
                               rng=rng)
        ng = (P + G - 1) // G
        ptr, adj = csr(ng, pose_pairs_to_groups(pairs, G))
        K = 6 if t % 7 == 0 else 0
        perm, cand, _, prod = order(hc, P, D, K, ptr, adj)
        check_perm(perm, P, G)
        assert prod[0] > 0
        assert prod[cand] <= prod[0], (t, prod)
        assert prod[cand] == prod[prod > 0].min()
        kinds.append(cand)
    assert any(c != 0 for c in kinds)


def scene_group_pairs(sc, G, active):
    """Group pairs of the projection part of S for a scene (incidences as the engine forms them)."""
    nat = np.cumsum(active) - 1
    nat[active == 0] = -1
    obs_lm, obs_pose = sc.obs_lm.astype(np.int64), sc.obs_pose.astype(np.int64)
    g = nat[obs_pose]
    ok = g >= 0
    g = np.where(ok, g // G, -1)
    out = []
    order_ = np.argsort(obs_lm, kind="stable")
    lm_s, g_s = obs_lm[order_], g[order_]
    bounds = np.r_[0, np.nonzero(np.diff(lm_s))[0] + 1, len(lm_s)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        u = np.unique(g_s[a:b])
        u = u[u >= 0]
        if len(u) > 1:
            i, j = np.triu_indices(len(u), 1)
            out.append(np.stack([u[i], u[j]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def test_multilap_route_auto_cuts_tile_products():
    """6 000 poses driven three times, 30 % of the places seen again: the model expects 0.027 x natural."""
    from ba_amd import scene
    lib = ctypes.CDLL(LIB) if os.path.exists(LIB) else None
    if lib is None:
        import __graft_entry__
        __graft_entry__.build()
        lib = ctypes.CDLL(LIB)
    sc = scene.make_revisit_scene(6000, 30000, laps=3, window=40, revisit_frac=0.3, seed=0)
    act = np.ones(sc.num_poses, dtype=np.int64)
    act[sc.anchor_poses] = 0
    D, G = 6, 32
    Pact = int(act.sum())
    ng = (Pact + G - 1) // G
    ptr, adj = csr(ng, scene_group_pairs(sc, G, act))
    perm, cand, _, prod = order(lib, Pact, D, 0, ptr, adj)
    check_perm(perm, Pact, G)
    assert cand != 0
    assert prod[cand] <= 0.1 * prod[0], prod
