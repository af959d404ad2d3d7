"""Soundness gate of the tile-factor assertions (tile_factor_cases.py), on the CPU: a plain float64 un-pivoted
sign-L D L^T passes every bound on every case of the grid the device runs, each of five subtly wrong factors
fails them, and the numpy symbolic elimination agrees with tile_symbolic_factor (ordering.h)."""
import ctypes
import os

import numpy as np
import pytest

import tile_factor_cases as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u8p = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_tile_factor.restype = ctypes.c_uint64
    return lib


@pytest.mark.parametrize("family", tf.FAMILIES)
def test_reference_factor_passes_every_bound(family, hc):
    worst_f = worst_s = 0.0
    for nt, n, sign, graded in tf.combos(family):
        c = tf.family_case(family, nt, n, sign, graded)
        # the symbolic elimination against the engine's (symmetric pattern in, lower factor pattern out)
        sym = np.ascontiguousarray(np.tril(c.tile_map) | np.tril(c.tile_map).T | np.eye(nt, dtype=np.uint8))
        hc.ba_hostcheck_tile_factor(nt, sym.ctypes.data_as(u8p))
        assert np.array_equal(sym, c.nzL), c.name
        rf, rs = tf.check_factor(c, *tf.reference_ldlt(c))
        worst_f, worst_s = max(worst_f, rf), max(worst_s, rs)
    print("%s: worst factor ratio %.3g, worst solve ratio %.3g" % (family, worst_f, worst_s))
    # (the bounds hold with a margin for a correct factor: what a wrong one has to exceed is 1)
    assert worst_f < 1.0 and worst_s < 1.0


def test_fill_in_families_change_the_pattern():
    """The families do what their names say at the tile level."""
    nt = 25
    pat = lambda f: tf.family_case(f, nt, 64 * nt, "spd", False)
    c = pat("reverse_arrow")
    assert c.tile_map.sum() < c.nzL.sum() == nt * (nt + 1) // 2       # fills completely
    c = pat("arrow")
    assert np.array_equal(c.tile_map, c.nzL)                          # no fill
    c = pat("loop")
    assert c.nzL[nt - 1].sum() == nt and c.tile_map[nt - 1].sum() == 3  # fill along the last row
    c = pat("blockdiag")
    assert any(c.nzL[j + 1:, j].sum() == 0 for j in range(nt - 1))    # columns with nothing below the diagonal
    c = pat("lone1")
    blocks = c.tile_map[:24, :24].reshape(12, 2, 12, 2).sum(axis=(1, 3))
    assert set(np.tril(blocks, -1)[np.tril_indices(12, -1)].tolist()) == {1}   # one live tile per 128x128 block of S
    c = pat("lone2")
    blocks = c.tile_map[:24, :24].reshape(12, 2, 12, 2).sum(axis=(1, 3))
    assert set(np.tril(blocks, -1)[np.tril_indices(12, -1)].tolist()) == {2}
    c = pat("superset")
    assert c.tile_map.sum() == nt * (nt + 1) // 2 and len(c.tiles) == 2 * nt - 1


# ---- mutated factors ------------------------------------------------------------------------------------------
def _fails(c, out, which):
    with pytest.raises(tf.FactorCheckError) as e:
        tf.check_factor(c, *out)
    assert e.value.which == which, str(e.value)
    return str(e.value)


MUTATION_CASES = [("band3", 24, 1536, "spd", False), ("reverse_arrow", 25, 1570, "every7", True),
                  ("random_a", 33, 2095, "trailing", False), ("loop", 5, 320, "onecol", True)]


@pytest.mark.parametrize("family,nt,n,sign,graded", MUTATION_CASES)
def test_mutated_factors_fail(family, nt, n, sign, graded):
    c = tf.family_case(family, nt, n, sign, graded)
    good = tf.reference_ldlt(c)
    tf.check_factor(c, *good)
    x, nzL, st, linvT, dsgn = good
    # a panel J with two nonzero tiles i >= k below the diagonal (the last such panel: least smoothing afterwards)
    J = max(j for j in range(nt) if c.nzL[j + 1:, j].sum() >= 2)
    rows = [i for i in range(J + 1, nt) if c.nzL[i, J]]
    # 1. one tile product left out of one trailing update
    _fails(c, tf.reference_ldlt(c, skip_product=(rows[1], rows[0], J)), "factor")
    _fails(c, tf.reference_ldlt(c, skip_product=(rows[1], rows[1], J)), "factor")
    # 2. one pivot sign flipped (the sign check sees it; without that check the factor bound does)
    for row in (0, n // 2, n - 1):
        d2 = dsgn.copy()
        d2[row] = -d2[row]
        _fails(c, (x, nzL, st, linvT, d2), "signs")
        c2 = tf.family_case(family, nt, n, sign, graded)
        c2.sgn[row] = -c2.sgn[row]
        _fails(c2, (x, nzL, st, linvT, d2), "factor")
    # 3. one entry of L off by 1e-11 relative.  The bound is relative to the row's |L| |L^T| |v|, so 1e-11 shows
    # where the entry carries more than gamma_(n+1) / 1e-11 (2 to 3 %) of its row: the diagonal of L does (these
    # matrices are diagonally dominant), perturbed here through linvT as the device keeps it.  The largest
    # sub-diagonal entry carries about 1 % of its row, inside the bound by construction at 1e-11; at 1e-9 it is out.
    l2 = linvT.copy()
    l2[J, 5, 5] *= 1.0 + 1e-11
    _fails(c, (x, nzL, st, l2, dsgn), "factor")
    sub = np.tril(st, -1)
    for t in range(nt):
        sub[64 * t:64 * t + 64, 64 * t:64 * t + 64] = 0.0
    r, q = np.unravel_index(np.argmax(np.abs(sub)), sub.shape)
    s2 = st.copy()
    s2[r, q] *= 1.0 + 1e-9
    _fails(c, (x, nzL, s2, linvT, dsgn), "factor")
    # 4. one tile of L written outside nzL
    out = np.argwhere((np.tril(np.ones((nt, nt)), -1) > 0) & (c.nzL == 0))
    if family != "reverse_arrow":  # (that one fills completely)
        i, k = out[len(out) // 2]
        s2 = st.copy()
        s2[64 * i + 3, 64 * k + 60] = 1e-300
        _fails(c, (x, nzL, s2, linvT, dsgn), "pattern")
        n2 = nzL.copy()
        n2[i, k] = 1
        _fails(c, (x, n2, st, linvT, dsgn), "pattern")
    # 5. the rhs row left un-updated by one panel
    _fails(c, tf.reference_ldlt(c, skip_rhs=J), "solve")
    _fails(c, tf.reference_ldlt(c, skip_rhs=0), "solve")


def test_relative_perturbation_raises_the_factor_ratio_far_above_one():
    """The margin on both sides: a correct factor sits well below 1; a diagonal entry of L off by delta = 1e-11
    moves (L D L^T v)_r by about 2 delta l_rr^2 |v_r| against a bound of gamma_(n+1) (l_rr^2 |v_r| + the rest of the
    row), so the ratio rises to 2 delta / gamma_(n+1) = 117 times the share of the diagonal term in its row."""
    c = tf.family_case("band3", 24, 1536, "every7", True)
    x, nzL, st, linvT, dsgn = tf.reference_ldlt(c)
    rf, rs = tf.check_factor(c, x, nzL, st, linvT, dsgn)
    assert rf < 0.25 and rs < 0.25
    linvT[9, 40, 40] *= 1.0 + 1e-11
    with pytest.raises(tf.FactorCheckError) as e:
        tf.check_factor(c, x, nzL, st, linvT, dsgn)
    ratio = float(str(e.value).split(" is ")[1].split(" times")[0])
    print("ratio before %.3g, after %.3g" % (rf, ratio))
    assert ratio > 10.0
