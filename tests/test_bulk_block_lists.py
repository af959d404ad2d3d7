"""The launch lists of the bulk LDL^T update (ba_amd/csrc/bulk_lists.h) on the CPU, through ba_hostcheck_bulk_lists.

A bulk launch of cholesky_solve covers the non-empty 128-blocks of its trailing triangle from a list instead of
starting a workgroup for every position.  The builder is compared here with a numpy restatement of the kernel's
mask rule (k_update128: tile column k of the panel [J, Jend) is active for block (R, C) when nz[i, k] | nz[i + 1, k]
and nz[c, k] | nz[c + 1, k], i = a_end + 2 R, c = a_end + 2 C), launch by launch, on

  * the seven patterns of test_bulk_update_schedule_gpu.CASES and dense96 (test_bulk_update_epilogue_gpu),
  * noblock48: a band of half-width 2 on 48 tiles, whose one 128-launch (a_end = 32, panel 0 .. 15) has no block,
  * oneblock48: the same band and tile (32, 5): that launch has exactly one block, (0, 0),
  * ring938: the circular band of the flagship's size (938 tiles, half-width 226) with panels of 16,

all with BA_HIP_KOUT = 16; the 48 .. 96-tile patterns with BA_HIP_BULK_FULL_M = 16 as the GPU tests run them.

Per launch: the entries that are no sentinels are exactly the blocks with a non-empty mask, each once and with its
mask; sentinels stand only at the end of their per-XCD sub-list (list position mod 8) and are at most 7 x 16 = 112;
the per-XCD counts are within 16 of each other (least-count dealing of items of at most 16); the entries of a 4x4
super-block are consecutive in one sub-list, in the grid launch's `within` order; the launches with a list are the
launches bulk_shape gives to the 128-block triangle kernel, no other.  Also: the grid of the new BulkKernel kind, the
byte budget, the BA_HIP_BULK_GRID switch, and that a plain float64 reference meets the bounds of
tile_factor_cases.check_factor on the two new patterns (soundness of the GPU test's pass condition).
"""
import ctypes

import numpy as np
import pytest

import test_bulk_update_epilogue_gpu as epi
import tile_factor_cases as tf
from helpers import hostcheck_lib

PANEL = 16
SENTINEL = 0xFFFFFFFF
U128, U128_LIST, U2_FULL, U2_CAPPED, U128_BLOCKS = range(5)
NEW_CASES = ("noblock48", "oneblock48")
SMALL = list(epi.CASES) + list(NEW_CASES)
RING_NT, RING_HW, RING_BLOCKS = 938, 226, 924579


def band_pairs(nt, hw):
    return [(i, j, "d") for i in range(nt) for j in range(max(0, i - hw), i)]


def build(name):
    """The cases of the GPU test by name (the new ones: 48 tiles, n ending inside the last tile)."""
    if name == "noblock48":
        return tf.make_case(48, 64 * 48 - 9, band_pairs(48, 2), (), False, 4400, None, "bulk-lists noblock48")
    if name == "oneblock48":
        return tf.make_case(48, 64 * 48 - 9, band_pairs(48, 2) + [(32, 5, "d")], (), False, 4401, None,
                            "bulk-lists oneblock48")
    return epi.build(name)


def ring_pattern():
    i = np.arange(RING_NT)[:, None]
    j = np.arange(RING_NT)[None, :]
    d = np.abs(i - j)
    return tf.symbolic((np.minimum(d, RING_NT - d) <= RING_HW) & (j <= i))


_PATTERNS = {}


def pattern(name):
    """(nzL, bulk_full_m) of a case, computed once."""
    if name not in _PATTERNS:
        _PATTERNS[name] = (ring_pattern(), 128) if name == "ring938" else (np.ascontiguousarray(build(name).nzL), 16)
    return _PATTERNS[name]


def chol_launch(op, row, strings=(None,), n_out=6):
    hc = hostcheck_lib()
    hc.ba_hostcheck_chol_launch.restype = ctypes.c_int
    a = np.ascontiguousarray(row, dtype=np.int64)
    out = np.full(n_out, -1, dtype=np.int64)
    s = (ctypes.c_char_p * len(strings))(*strings)
    rc = hc.ba_hostcheck_chol_launch(op, 1, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), s,
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    assert rc == 0, rc
    return [int(v) for v in out]


def lists(nz, kout=PANEL, bulk_full_m=128, budget=-1, no128=0, full_always=0, bulk_grid=0, dense=0, nblk=None):
    """build_bulk_lists: (built, launches as dicts with their entries (R, C, mask) as an int64 array)."""
    hc = hostcheck_lib()
    hc.ba_hostcheck_bulk_lists.restype = ctypes.c_int64
    nblk = nz.shape[0] if nblk is None else nblk
    hdr = np.array([nblk, kout, no128, bulk_full_m, full_always, bulk_grid, dense], dtype=np.uint32)
    cap = 4 + 14 * (nblk // kout + 2) + 3 * (8 * 16 * (nblk // kout + 2) + (nblk // kout + 2) * (nblk // 2 + 4) ** 2 // 2)
    out = np.zeros(cap, dtype=np.int64)
    p = None if nz is None else np.ascontiguousarray(nz, dtype=np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    n = hc.ba_hostcheck_bulk_lists(hdr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), p, ctypes.c_int64(budget),
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_uint64(cap))
    assert n >= 4, n
    built, nl, total, ne = (int(v) for v in out[:4])
    assert n == 4 + 14 * nl + 3 * ne
    ent = out[4 + 14 * nl:n].reshape(ne, 3)
    launches = []
    for row in out[4:4 + 14 * nl].reshape(nl, 14):
        l = dict(zip(("a_end", "J", "Jend", "first", "len", "blocks"), (int(v) for v in row[:6])))
        l["xcd_blocks"] = [int(v) for v in row[6:]]
        l["entries"] = ent[l["first"]:l["first"] + l["len"]]
        launches.append(l)
    assert sum(l["len"] for l in launches) == ne and sum(l["blocks"] for l in launches) == total
    return built, launches


def solve_launches(nblk, kout, bulk_full_m):
    """cholesky_solve's loop: (a_end, J, Jend, kernel kind today) of every bulk launch."""
    out = []
    for J in range(0, nblk, kout):
        Jend = min(J + kout, nblk)
        if Jend >= nblk:
            break
        a_end = min(Jend + kout, nblk)
        if a_end >= nblk:
            continue
        full = int(nblk - a_end >= bulk_full_m)
        out.append((a_end, J, Jend, chol_launch(3, [nblk, a_end, full, 1, 1, 0, 0, 0, 3])[0]))
    return out


def expected_blocks(nz, a_end, J, Jend):
    """The kernel's rule, restated: arrays R, C, mask of the blocks C <= R < m2 with a non-empty mask, sorted by (R, C)."""
    nblk = nz.shape[0]
    m2 = (nblk - a_end) // 2
    rows = a_end + 2 * np.arange(m2)
    U = (nz[rows, J:Jend] | nz[rows + 1, J:Jend]).astype(bool)                 # [m2, columns of the panel]
    w = (1 << np.arange(Jend - J, dtype=np.int64))
    M = ((U[:, None, :] & U[None, :, :]) * w).sum(axis=2)                      # mask of (R, C)
    R, C = np.nonzero(np.tril(M != 0))
    return R, C, M[R, C]


def check_launch(nz, l):
    R, C, M = expected_blocks(nz, l["a_end"], l["J"], l["Jend"])
    e = l["entries"]
    assert l["len"] % 8 == 0 and e.shape[0] == l["len"]
    real = e[:, 0] != SENTINEL
    # exactly the non-empty blocks, each once, each with its mask
    got = e[real]
    order = np.lexsort((got[:, 1], got[:, 0]))
    assert np.array_equal(got[order, 0], R) and np.array_equal(got[order, 1], C) and np.array_equal(got[order, 2], M)
    assert l["blocks"] == R.size
    # sentinels: whole entries, at the end of their sub-list only, at most 7 x 16
    assert np.all(e[~real, 1] == SENTINEL) and np.all(e[~real, 2] == 0)
    assert (~real).sum() <= 112
    counts = []
    for x in range(8):
        sub, r = e[x::8], real[x::8]
        counts.append(int(r.sum()))
        assert np.all(r[:counts[-1]]) and not np.any(r[counts[-1]:])
        # a super-block's entries are consecutive, in the `within` order of the grid launch
        sb = (sub[r, 0] // 4) * (1 << 20) + sub[r, 1] // 4
        within = (sub[r, 0] % 4) * 4 + sub[r, 1] % 4
        starts = np.nonzero(np.diff(sb, prepend=-1))[0]
        assert np.unique(sb[starts]).size == starts.size                       # one run per super-block
        inside = np.ones(sb.size, dtype=bool)
        inside[starts] = False
        assert np.all(np.diff(within, prepend=0)[inside] > 0)
        # ... and the super-blocks of a sub-list keep the triangular order
        t = (sub[r, 0] // 4) * (sub[r, 0] // 4 + 1) // 2 + sub[r, 1] // 4
        assert np.all(np.diff(t[starts]) > 0)
    assert counts == l["xcd_blocks"] and max(counts) - min(counts) <= 16
    assert l["len"] == 8 * max(counts)
    return R.size


@pytest.mark.parametrize("name", SMALL + ["ring938"])
def test_lists_are_the_nonempty_blocks(name):
    nz, full_m = pattern(name)
    built, launches = lists(nz, bulk_full_m=full_m)
    assert built == 1
    today = solve_launches(nz.shape[0], PANEL, full_m)
    # every launch of the 128-block triangle kernel has a list, no other launch has one
    assert [(l["a_end"], l["J"], l["Jend"]) for l in launches] == [t[:3] for t in today if t[3] == U128]
    total = sum(check_launch(nz, l) for l in launches)
    worst = max(launches, key=lambda l: l["len"] - l["blocks"])
    print("%s: %d launches, %d blocks, at most %d sentinels, XCD counts within %d" % (
        name, len(launches), total, worst["len"] - worst["blocks"],
        max(max(l["xcd_blocks"]) - min(l["xcd_blocks"]) for l in launches)))
    if name == "ring938":
        assert len(launches) == 49 and total == RING_BLOCKS
        started = sum(chol_launch(3, [RING_NT, l["a_end"], 1, 1, 1, 0, 0, 0, 3])[1] for l in launches)
        print("ring938: the grid launches start %d workgroups" % started)
    if name == "noblock48":
        assert [(l["a_end"], l["len"], l["blocks"]) for l in launches] == [(32, 0, 0)]
    if name == "oneblock48":
        assert [(l["a_end"], l["len"], l["blocks"]) for l in launches] == [(32, 8, 1)]
        assert launches[0]["entries"][0].tolist() == [0, 0, sum(1 << k for k in range(5, 16))]
    if name == "dense96":
        assert [l["a_end"] for l in launches] == [32, 48, 64, 80]


def test_launch_kinds_follow_the_switches():
    nz, _ = pattern("nt50")
    assert lists(nz, bulk_full_m=128)[1] == []                      # capped launches: the 64-tile kernel, no list
    assert len(lists(nz, bulk_full_m=128, full_always=1)[1]) == 1   # BA_HIP_NO_LOOKAHEAD / BA_HIP_BULK_FULL
    assert lists(nz, bulk_full_m=16, no128=1) == (1, [])
    assert lists(nz, bulk_full_m=16, bulk_grid=1) == (0, [])        # BA_HIP_BULK_GRID, BA_HIP_DENSE, no pattern:
    assert lists(nz, bulk_full_m=16, dense=1) == (0, [])            # nothing is built, the grid launch stays
    assert lists(None, bulk_full_m=16, nblk=50) == (0, [])
    assert lists(nz, kout=65, bulk_full_m=16) == (0, [])            # the kernel's mask is one ballot of 64 columns


def test_budget_fallback():
    nz, full_m = pattern("dense96")
    built, launches = lists(nz, bulk_full_m=full_m)
    need = 8 * sum(l["len"] for l in launches)
    assert built == 1 and need > 0
    assert lists(nz, bulk_full_m=full_m, budget=need)[0] == 1
    assert lists(nz, bulk_full_m=full_m, budget=need - 1) == (0, [])
    # the default budget holds the flagship's lists with room to spare and is a small part of its S (32 GB)
    ring = sum(l["len"] for l in lists(*pattern("ring938"))[1])
    assert 4 * 8 * ring <= (64 << 20) <= 32e9 / 400


@pytest.mark.parametrize("nblk,a_end", [(938, 32), (938, 904), (50, 32), (49, 32), (48, 32)])
def test_grid_of_the_list_kind(nblk, a_end):
    grid_launch = chol_launch(3, [nblk, a_end, 1, 1, 1, 0, 0, 0, 3])
    assert grid_launch[0] == U128
    m = nblk - a_end
    nrow64 = (m * (1 + (m & 1)) + 7) // 8 * 8
    for longest in (0, 1, 17, 3000):
        kind, grid, n64, m2, sbl, swzf = chol_launch(9, [nblk, a_end, 1, 1, 1, 0, 0, 0, 3, 8 * longest, 0])
        assert (kind, grid, n64) == (U128_BLOCKS, nrow64 + 8 * longest, nrow64)
        assert [n64, m2, sbl, swzf] == grid_launch[2:]                 # the leading 64-tile workgroups stay
    base = [nblk, a_end, 1, 1, 1, 0, 0, 0, 3]
    assert chol_launch(9, base + [-1, 0]) == grid_launch               # no list
    assert chol_launch(9, base + [800, 1]) == grid_launch              # BA_HIP_BULK_GRID
    assert chol_launch(9, [nblk, a_end, 0, 1, 1, 0, 0, 0, 3, 800, 0])[0] == U2_CAPPED
    assert chol_launch(9, [nblk, a_end, 1, 1, 1, 0, 0, 1, 3, 800, 0])[0] == U2_FULL
    # the distributed solve's launches are what they were, list or not
    for row in ([nblk, a_end, 1, 4, 2, 1, 5, 0, 3], [nblk, a_end, 1, 4, 2, 0, 0, 0, 3], [nblk, a_end, 1, 4, 3, 1, 5, 0, 3]):
        assert chol_launch(9, row + [800, 0]) == chol_launch(3, row)


def test_the_switch_is_parsed_as_a_process_switch():
    """Operation 8 of ba_hostcheck_chol_launch: BA_HIP_BULK_GRID set (any value) / unset."""
    for val, want in ((None, 0), (b"1", 1), (b"0", 1), (b"", 1)):
        assert chol_launch(8, [0], (val,), n_out=1) == [want]


@pytest.mark.parametrize("name", NEW_CASES)
def test_reference_meets_the_bounds(name):
    """Soundness gate of the GPU test: a plain float64 reference passes check_factor on the two new patterns."""
    c = build(name)
    rf, rs = tf.check_factor(c, *tf.reference_ldlt(c))
    print("%s: reference factor ratio %.3g, solve ratio %.3g" % (c.name, rf, rs))
    assert rf < 1.0 and rs < 1.0
