"""The K loop of the bulk trailing update k_update128 (k_chol.hip) at chosen trip counts.

The loop walks the panel's tile columns through a bit mask: per 128x128 block the tile columns where either
of its two tile rows AND either of its two tile columns is structurally nonzero.  `while (mask)` runs once per
column but the last, which is a peeled copy; the operand chunk after next is prefetched from the NEXT set bit
(`knext`).  These cases choose the masks of the blocks of ONE launch, the first bulk launch with
BA_HIP_KOUT = 16 and the 128-path threshold lowered to 16 tile rows (BA_HIP_BULK_FULL_M = 16): panel = tile
columns 0-15, a_end = 32, trailing tile rows 32 .. nt - 1.

Shapes: 48, 49, 50 and 51 tiles give 16 .. 19 trailing tile rows, i.e. 8 or 9 128-blocks per side with and
without the odd leftover tile row (which rides along as 64-tiles), n ending inside the last tile: the smallest
sizes at which that launch goes through the 128-path.  54 tiles: a last panel of 6 tile columns (11 128-blocks
per side in the first launch).

Patterns: the panel's own square is block-diagonal (diagonal tiles only), so no fill appears inside the
panel and the column sets COLS given to the tile rows from 16 on survive unchanged in L.  With U_R the union of
the sets of the two tile rows of block row R, block (R, C) of the launch has mask U_R & U_C (U_R on the
diagonal).  The table below gives, in one launch,
    (a) one common column   blocks (2, 0) {3}, (2, 2) {3}, (3, 2) {3}, (7, 1) {0}: the loop body is skipped
    (b) two                 blocks (3, 0), (3, 3) {3, 9}: one loop trip
    (c) every other column  blocks (1, 0), (1, 1): holes in the mask, knext jumps
    (d) all 16              blocks (0, 0), (6, 0)
    (e) two tile rows with different sets (structurally zero tiles inside the product)
                            blocks (4, 0) {0,1,2,3} | {8,9}, (5, 0) {5} | {12}, (5, 1) {12}, (7, 0)
    (f) diagonal blocks     (R, R) of every kind above
and empty masks (blocks (2, 1), (3, 1)).  The tile rows 16 .. 31 repeat the table, so the rectangle variant
below the next panel (k_update128<true>) meets the same masks.

Indefinite systems: sign "trailing" makes the rows from n / 2 on negative, i.e. the tile columns from 24 on.  The
K range of the 128-launches at these sizes is the tile columns 0 .. 15, so that case runs the K loop with
negative pivots everywhere else but does not send a block through the 64-tile fallback; the case "negpanel"
(negative pivots in tile column 5 of the panel) does, for every block whose mask is not empty.

Every case runs in a child process of its own (the threshold switch is read once per process) with its own
time limit; a child that ends on a signal or its limit fails the test and is not run again.  Pass condition: the
componentwise backward-error ratios of tile_factor_cases.check_factor below 1 and two identical calls bitwise
equal.  The CPU test in this file shows that a plain float64 reference meets the bounds on every case and that
leaving out ONE tile product of a block of kind (a), (c) or (e) does not.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import tile_factor_cases as tf  # noqa: E402

PANEL = 16      # BA_HIP_KOUT
A_END = 32      # first tile row of the first bulk launch
ALL = tuple(range(16))
EVEN = tuple(range(0, 16, 2))
ODD = tuple(range(1, 16, 2))
# column sets of the tile rows A_END + j (and 16 + j), j = 0 .. 19: two rows per 128-block row R = j // 2
COLS = [
    ALL, ALL,                   # R0  U = all 16
    EVEN, EVEN,                 # R1  U = every other column
    (3,), (3,),                 # R2  U = {3}
    (3, 9), (3, 9),             # R3  U = {3, 9}
    (0, 1, 2, 3), (8, 9),       # R4  different sets: U = {0, 1, 2, 3, 8, 9}
    (5,), (12,),                # R5  different sets: U = {5, 12}
    ALL, (15,),                 # R6  U = all 16, one row nearly empty
    ODD, (0,),                  # R7  U = the odd columns and 0
    (14, 15), ALL,              # R8  (from 50 tiles on; at 49 tiles row 48 is the odd 64-tile row)
    EVEN, (7,),                 # (51 tiles: row 50 is the odd 64-tile row; 54 tiles: R9)
    (2, 3, 4), ODD,             # (54 tiles: R10)
]


def pairs_for(nt):
    out = []
    for r in range(PANEL, nt):
        j = (r - PANEL) % 16 if r < A_END else r - A_END
        out += [(r, k, "d") for k in COLS[j]]
    return out


# name -> (tile count, n, negative rows)
CASES = {
    "nt48": (48, 64 * 48 - 17, "spd"),
    "nt49": (49, 64 * 48 + 1, "spd"),          # the last tile holds one row
    "nt50": (50, 64 * 50 - 30, "spd"),
    "nt51": (51, 64 * 51 - 63, "spd"),
    "short_last_panel": (54, 64 * 54 - 23, "spd"),
    "trailing": (48, 64 * 48 - 17, "trailing"),
    "negpanel": (49, 64 * 49 - 5, "negpanel"),
}
# products left out by the soundness gate: (tile row, tile column, panel column) of blocks of kind (a), (c), (e)
MUTATIONS = {"a": (36, 32, 3), "c": (34, 32, 4), "e": (40, 33, 2)}


def build(name):
    nt, n, sign = CASES[name]
    if sign == "negpanel":
        neg = np.arange(64 * 5, 64 * 6, 3)
    else:
        neg = tf.neg_rows(sign, nt, n)
    return tf.make_case(nt, n, pairs_for(nt), neg, False, 4200 + sorted(CASES).index(name), None, "bulk-schedule " + name)


def block_mask(c, R, C):
    """The tile columns k_update128 forms for block (R, C) of the first bulk launch."""
    i, k = A_END + 2 * R, A_END + 2 * C
    rows = c.nzL[i, :PANEL] | (c.nzL[i + 1, :PANEL] if i + 1 < c.nt else 0)
    cols = c.nzL[k, :PANEL] | c.nzL[k + 1, :PANEL]
    return tuple(np.nonzero(rows & cols)[0].tolist())


def test_patterns_survive_and_give_the_masks():
    c = build("nt50")
    assert c.nzL[:PANEL, :PANEL].sum() == PANEL                      # no fill inside the panel's square
    for r in range(PANEL, c.nt):
        j = (r - PANEL) % 16 if r < A_END else r - A_END
        assert tuple(np.nonzero(c.nzL[r, :PANEL])[0].tolist()) == COLS[j]
    assert block_mask(c, 2, 0) == (3,) and block_mask(c, 2, 2) == (3,) and block_mask(c, 7, 1) == (0,)   # (a)
    assert block_mask(c, 3, 0) == (3, 9) and block_mask(c, 3, 3) == (3, 9)                               # (b)
    assert block_mask(c, 1, 0) == EVEN and block_mask(c, 1, 1) == EVEN                                   # (c)
    assert block_mask(c, 0, 0) == ALL and block_mask(c, 6, 0) == ALL                                     # (d)
    assert block_mask(c, 4, 0) == (0, 1, 2, 3, 8, 9) and block_mask(c, 5, 0) == (5, 12)                  # (e)
    assert block_mask(c, 5, 1) == (12,) and block_mask(c, 4, 4) == (0, 1, 2, 3, 8, 9)
    assert block_mask(c, 2, 1) == () and block_mask(c, 3, 1) == ()
    assert block_mask(c, 8, 0) == ALL and block_mask(c, 8, 2) == (3,)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_meets_the_bounds(name):
    """Soundness gate: a plain float64 reference passes check_factor on every case."""
    c = build(name)
    rf, rs = tf.check_factor(c, *tf.reference_ldlt(c))
    print("%s: reference factor ratio %.3g, solve ratio %.3g" % (c.name, rf, rs))
    assert rf < 1.0 and rs < 1.0


@pytest.mark.parametrize("kind", list(MUTATIONS))
def test_one_product_left_out_fails(kind):
    """... and a factor that lacks one tile product of a block of kind (a), (c) or (e) does not."""
    c = build("nt48")
    i, k, J = MUTATIONS[kind]
    assert c.nzL[i, J] and c.nzL[k, J]
    with pytest.raises(tf.FactorCheckError) as e:
        tf.check_factor(c, *tf.reference_ldlt(c, skip_product=(i, k, J)))
    assert e.value.which == "factor", str(e.value)


def run_case(name):
    """Child process: the device factor of one case, twice."""
    from ba_amd import hipapi
    c = build(name)
    a = tf.lower_dense(c)
    eng = hipapi.Engine(1, 6)
    try:
        outs = []
        for _ in range(2):
            x, rc, nzL, st, linvT, dsgn = eng.tile_solve(a, c.b, c.tile_map, keep_factor=True)
            assert rc == 0, c.name
            outs.append((x, nzL, st, linvT, dsgn))
        for what, p, q in zip(("x", "nzL", "storage", "linvT", "dsgn"), outs[0], outs[1]):
            assert p.tobytes() == q.tobytes(), "%s: %s differs between two identical calls" % (c.name, what)
        rf, rs = tf.check_factor(c, *outs[0])
    finally:
        eng.close()
    print("RATIO %s: factor %.3g solve %.3g" % (name, rf, rs))
    assert rf < 1.0 and rs < 1.0
    print("CASE-OK " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_factor(name):
    env = dict(os.environ, BA_HIP_BULK_FULL_M="16", BA_HIP_KOUT="16")
    for k in ("BA_HIP_LEFT_MIN_TILES", "BA_HIP_SQUARE", "BA_HIP_SQ_W", "BA_HIP_NO128", "BA_HIP_NO_LOOKAHEAD",
              "BA_HIP_BULK_FULL"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True,
                       timeout=120)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("RATIO")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "CASE-OK " + name in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    run_case(sys.argv[1])
