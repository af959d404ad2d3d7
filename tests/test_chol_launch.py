"""Host decisions of the LDL^T solve (ba_amd/csrc/chol_launch.h) on the CPU: switch parsing, the launch shapes, the
layout of the factor work space and the key of the distributed plan, through ba_hostcheck_chol_launch.

The shapes are compared with a restatement of the formulas as they stood inside launch_next_panel_update,
launch_bulk_update and the rectangle branch of cholesky_solve_dist before the header existed (REF_* below): the
header must choose the same kernels and the same grids."""
import ctypes

import numpy as np
import pytest

from helpers import hostcheck_lib

PROCESS = ("NO128", "NO_LOOKAHEAD", "BULK_FULL", "DENSE", "NO_DIST_SOLVE", "SBL", "BULK_FULL_M")
CALL = ("KOUT", "LEFT_MIN_TILES", "SQUARE", "SQ_W", "DIST_LAYOUT", "DENSE_SCATTER", "TRACE_FILE")
FIELDS = ("no128", "no_lookahead", "bulk_full", "dense", "no_dist_solve", "sbl", "rect_min_rows", "bulk_full_m", "kout",
          "left_min_tiles", "square", "sq_w", "dist_layout", "dense_scatter", "trace_file")
WIDTH = {1: (2, 2), 2: (7, 5), 3: (9, 6), 4: (1, 6)}   # op: columns in, columns out
U128, U128_LIST, U2_FULL, U2_CAPPED = range(4)


def call(op, rows=None, strings=(), n_out=None):
    hc = hostcheck_lib()
    hc.ba_hostcheck_chol_launch.restype = ctypes.c_int
    a = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    n = 1 if op in (0, 5) else a.size // WIDTH[op][0]
    out = np.zeros(n * (n_out or WIDTH[op][1]), dtype=np.int64)
    s = (ctypes.c_char_p * max(len(strings), 1))(*[None if v is None else str(v).encode() for v in strings])
    rc = hc.ba_hostcheck_chol_launch(op, n, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), s,
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    assert rc == 0, rc
    return out.reshape(n, -1)


def switches(nblk=100, **env):
    """the parsed switches for a solve of nblk tiles with BA_HIP_<name> = value for every keyword"""
    assert set(env) <= set(PROCESS + CALL)
    out = call(0, [nblk], [env.get(k) for k in PROCESS + CALL], n_out=len(FIELDS))
    return dict(zip(FIELDS, (int(v) for v in out[0])))


def test_unknown_op():
    hc = hostcheck_lib()
    hc.ba_hostcheck_chol_launch.restype = ctypes.c_int
    z = (ctypes.c_int64 * 1)(0)
    assert hc.ba_hostcheck_chol_launch(6, 1, z, None, z) == -1


# ---- 1. switch parsing: the table of DESIGN.md 9.1a ----------------------------------------------------------------
def test_defaults():
    assert switches(100) == dict(no128=0, no_lookahead=0, bulk_full=0, dense=0, no_dist_solve=0, sbl=3,
                                 rect_min_rows=128, bulk_full_m=128, kout=4, left_min_tiles=512, square=0, sq_w=4,
                                 dist_layout=0, dense_scatter=0, trace_file=0)


@pytest.mark.parametrize("name,field", [("NO128", "no128"), ("NO_LOOKAHEAD", "no_lookahead"), ("BULK_FULL", "bulk_full"),
                                        ("DENSE", "dense"), ("NO_DIST_SOLVE", "no_dist_solve"),
                                        ("DENSE_SCATTER", "dense_scatter"), ("DIST_LAYOUT", "dist_layout"),
                                        ("TRACE_FILE", "trace_file")])
@pytest.mark.parametrize("value", ["1", "0", ""])
def test_presence_switches(name, field, value):
    """set is set, whatever the value; nothing else moves"""
    want = dict(switches(100), **{field: 1})
    assert switches(100, **{name: value}) == want


@pytest.mark.parametrize("nblk,want", [(1, 4), (255, 4), (256, 8), (399, 8), (400, 16), (938, 16)])
@pytest.mark.parametrize("value", [None, "0", ""])
def test_kout_by_size(nblk, want, value):
    assert switches(nblk, KOUT=value)["kout"] == want


@pytest.mark.parametrize("nblk", [1, 300, 938])
def test_kout_given(nblk):
    assert [switches(nblk, KOUT=str(k))["kout"] for k in (1, 3, 16, 40)] == [1, 3, 16, 40]


@pytest.mark.parametrize("value,want", [(None, 3), ("2", 2), ("0", 0), ("4", 4)])
def test_sbl(value, want):
    assert switches(SBL=value)["sbl"] == want


@pytest.mark.parametrize("value,rect_min_rows,bulk_full_m", [(None, 128, 128), ("8", 16, 8), ("16", 16, 16), ("17", 17, 17),
                                                              ("0", 16, 0), ("200", 200, 200)])
def test_bulk_full_m_has_two_readings(value, rect_min_rows, bulk_full_m):
    sw = switches(BULK_FULL_M=value)
    assert (sw["rect_min_rows"], sw["bulk_full_m"]) == (rect_min_rows, bulk_full_m)


@pytest.mark.parametrize("value,want", [(None, 512), ("0", 1), ("-3", 1), ("1", 1), ("40", 40), ("600", 600)])
def test_left_min_tiles(value, want):
    assert switches(LEFT_MIN_TILES=value)["left_min_tiles"] == want


@pytest.mark.parametrize("value,nblk,want", [(None, 100, 0), ("0", 100, 0), ("1", 100, 1), ("2", 511, 1), ("1", 512, 0),
                                             ("1", 938, 0), ("", 100, 0)])
def test_square_only_below_512_tiles(value, nblk, want):
    assert switches(nblk, SQUARE=value)["square"] == want


@pytest.mark.parametrize("value,want", [(None, 4), ("0", 1), ("1", 1), ("2", 2), ("3", 3), ("4", 4), ("9", 4)])
def test_sq_w_clamped(value, want):
    assert switches(SQ_W=value)["sq_w"] == want


@pytest.mark.parametrize("left_min,nblk,want", [(512, 511, (0, 4)), (512, 512, (1, 8)), (512, 938, (1, 8)), (1, 1, (1, 8)),
                                                (40, 39, (0, 4)), (40, 40, (1, 8))])
def test_chain_shape(left_min, nblk, want):
    assert tuple(call(1, [nblk, left_min])[0]) == want


# ---- 2. shapes against the formulas they replace -------------------------------------------------------------------
def REF_rect(dist, nblk, c0, ncols, G, no128, bulk_full_m_env):
    """launch_next_panel_update (dist = 0: c0 = first column of the next panel) and the rectangle branch of
    cholesky_solve_dist (dist = 1: c0 is its c1), arrays in, columns use128 m2 rect_cols nrow64 grid out"""
    min_rows = 128 if bulk_full_m_env is None else max(16, bulk_full_m_env)
    r0 = c0 + ncols
    m = nblk - r0
    even = (ncols % 2 == 0) & (c0 % 2 == 0)
    use = np.where(dist == 1, (m >= 16) & even & (G % 2 == 0), (r0 + min_rows <= nblk) & even) & (not no128)
    m2, rect_cols = m // 2, ncols // 2
    nrow64 = (ncols * (1 + (m & 1)) + 7) // 8 * 8
    out = np.stack([np.ones_like(m), m2, rect_cols, nrow64, nrow64 + m2 * rect_cols], axis=1)
    return out * use[:, None]


def REF_bulk(nblk, a_end, full, own_n, own_G, have_pairs, npairs, no128, sbl):
    """launch_bulk_update: columns kernel grid nrow64 m2 sbl swzf"""
    m = nblk - a_end
    big = (full == 1) & (m >= 16) & (a_end % 2 == 0) & ((own_n <= 1) | (own_G % 2 == 0)) & (not no128)
    m2, sbe2 = m // 2, 4
    nsr = (m2 + sbe2 - 1) // sbe2
    nsb = nsr * (nsr + 1) // 2
    nrow64 = (m * (1 + (m & 1)) + 7) // 8 * 8
    listed = (have_pairs == 1) & (own_n > 1) & (a_end % own_G == 0)
    per = (own_G // 2) * (own_G // 2)
    grid128 = np.where(listed, nrow64 + npairs * per, nrow64 + (nsb + 7) // 8 * 8 * sbe2 * sbe2)
    sbe = 1 << sbl
    nsr1 = (m + 1 + sbe - 1) // sbe
    nsb1 = nsr1 * (nsr1 + 1) // 2
    grid1 = (nsb1 + 7) // 8 * 8 * sbe * sbe
    two = np.full_like(m, 2)
    o128 = np.stack([np.where(listed, U128_LIST, U128), grid128, nrow64, m2, two, 0 * m], axis=1)
    o64 = np.stack([np.where(full == 1, U2_FULL, U2_CAPPED), grid1, 0 * m, 0 * m, 0 * m + sbl, 0 * m + (1 | sbl << 8)], axis=1)
    return np.where(big[:, None], o128, o64)


SIZES = list(range(1, 141)) + [469, 938]
WIDTHS = {"auto": None, "kout3": 3, "kout4": 4, "kout8": 8, "kout16": 16}
SWITCH_SETS = {"default": {}, "no128": {"NO128": "1"}, "bulk_full_m16": {"BULK_FULL_M": "16"},
               "bulk_full": {"BULK_FULL": "1"}, "sbl2": {"SBL": "2"}}


def panel_positions(width):
    """(nblk, first column, columns) of every next panel the solve visits at every size: panels of `width` tiles (None:
    by size), the last one ragged — the same walk in cholesky_solve (J, Jend, a_end) and in build_dist_plan (c0, c1, n1)"""
    rows = []
    for nblk in SIZES:
        k = width or (16 if nblk >= 400 else 8 if nblk >= 256 else 4)
        for J in range(0, nblk, k):
            Jend = min(J + k, nblk)
            if Jend >= nblk:
                break
            rows.append((nblk, Jend, min(Jend + k, nblk) - Jend))
    return np.array(rows, dtype=np.int64)


def cross(a, *lists):
    """every row of a with every combination of the values in lists, as extra columns"""
    for vals in lists:
        v = np.asarray(vals, dtype=np.int64)
        a = np.concatenate([np.repeat(a, len(v), axis=0), np.tile(v, len(a))[:, None]], axis=1)
    return a


def check_rect(rows, sw, env):
    """rows: dist nblk c0 ncols G"""
    full = np.concatenate([rows, np.full((len(rows), 1), sw["no128"]), np.full((len(rows), 1), sw["rect_min_rows"])], axis=1)
    got = call(2, full)
    v = env.get("BULK_FULL_M")
    want = REF_rect(*rows.T, "NO128" in env, None if v is None else int(v))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (rows[bad[0]], got[bad[0]], want[bad[0]])
    return got


def check_bulk(rows, sw, env):
    """rows: nblk a_end full own_n own_G have_pairs npairs"""
    full = np.concatenate([rows, np.full((len(rows), 1), sw["no128"]), np.full((len(rows), 1), sw["sbl"])], axis=1)
    got = call(3, full)
    want = REF_bulk(*rows.T, "NO128" in env, int(env.get("SBL", 3)))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (rows[bad[0]], got[bad[0]], want[bad[0]])
    return got


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("switch_set", SWITCH_SETS)
def test_single_gpu_shapes_at_every_panel(switch_set, width):
    env = SWITCH_SETS[switch_set]
    sw = switches(**env)
    pos = panel_positions(WIDTHS[width])
    rect = check_rect(cross(np.concatenate([np.zeros((len(pos), 1), dtype=np.int64), pos], axis=1), [1]), sw, env)
    a = pos[pos[:, 1] + pos[:, 2] < pos[:, 0]]   # a bulk update only where something lies right of the next panel
    bulk = check_bulk(cross(np.stack([a[:, 0], a[:, 1] + a[:, 2]], axis=1), [0, 1], [1], [1], [0], [0]), sw, env)
    if switch_set == "no128":
        assert not rect[:, 0].any() and (bulk[:, 0] >= U2_FULL).all()
    elif width != "kout3":
        assert rect[:, 0].any() and (bulk[:, 0] == U128).any() and (bulk[:, 0] == U2_CAPPED).any()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("switch_set", SWITCH_SETS)
def test_distributed_shapes_at_every_panel(switch_set, width):
    env = SWITCH_SETS[switch_set]
    sw = switches(**env)
    pos = panel_positions(WIDTHS[width])
    rect = check_rect(cross(np.concatenate([np.ones((len(pos), 1), dtype=np.int64), pos], axis=1), [3, 4, 5, 16]), sw, env)
    a = pos[pos[:, 1] + pos[:, 2] < pos[:, 0]]
    bulk = check_bulk(cross(np.stack([a[:, 0], a[:, 1] + a[:, 2]], axis=1), [0, 1], [1, 2, 8], [3, 4, 5, 16], [0, 1], [7]),
                      sw, env)
    if switch_set != "no128" and width != "kout3":
        assert rect[:, 0].any() and {U128, U128_LIST, U2_FULL, U2_CAPPED} == set(bulk[:, 0])


# the smallest shapes at which the formulas can go wrong: (nblk, c0, ncols) of the next panel; the bulk update starts
# at a_end = c0 + ncols
EDGES = {
    "m_odd": (45, 4, 4), "m_even": (46, 4, 4),
    "a_end_odd": (60, 3, 4), "c0_odd_a_end_even": (60, 3, 3), "ncols_odd": (60, 4, 3),
    "m_15": (23, 4, 4), "m_16": (24, 4, 4), "m_17": (25, 4, 4),
    "rows_127": (143, 8, 8), "rows_128": (144, 8, 8), "rows_129": (145, 8, 8),
    "ragged_last_panel_odd": (23, 16, 7), "ragged_last_panel_even": (22, 16, 6), "nothing_below": (24, 16, 8),
    "one_row_below": (25, 16, 8), "m_0_bulk": (8, 4, 4),
}


@pytest.mark.parametrize("switch_set", SWITCH_SETS)
@pytest.mark.parametrize("edge", EDGES)
def test_shape_edges(edge, switch_set):
    env = SWITCH_SETS[switch_set]
    sw = switches(**env)
    nblk, c0, ncols = EDGES[edge]
    rect = check_rect(np.concatenate([cross(np.array([[0]]), [nblk], [c0], [ncols], [1]),
                                      cross(np.array([[1]]), [nblk], [c0], [ncols], [3, 4, 5, 16])]), sw, env)
    bulk = check_bulk(cross(np.array([[nblk, c0 + ncols]]), [0, 1], [1, 2, 8], [3, 4, 5, 16], [0, 1], [0, 7]), sw, env)
    if switch_set == "default":   # what the edge is about, stated once
        single, dist_g4 = rect[0, 0], rect[2, 0]
        full_single = bulk[3 * 4 * 2 * 2, 0]   # the first row with full = 1: own_n = 1, no pairs
        want = {"m_odd": (0, 1, U128), "m_even": (0, 1, U128), "a_end_odd": (0, 0, U2_FULL),
                "c0_odd_a_end_even": (0, 0, U128), "ncols_odd": (0, 0, U2_FULL), "m_15": (0, 0, U2_FULL),
                "m_16": (0, 1, U128), "m_17": (0, 1, U128), "rows_127": (0, 1, U128), "rows_128": (1, 1, U128),
                "rows_129": (1, 1, U128), "ragged_last_panel_odd": (0, 0, U2_FULL),
                "ragged_last_panel_even": (0, 0, U2_FULL), "nothing_below": (0, 0, U2_FULL),
                "one_row_below": (0, 0, U2_FULL), "m_0_bulk": (0, 0, U2_FULL)}[edge]
        assert (single, dist_g4, full_single) == want


# ---- 3. the work space ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 2, 33, 938])
def test_factor_work_layout(nblk):
    """pivot signs | linvT | factor packets | colneg, as the five places that carved it by hand had it"""
    NB, NOPV = 64, 40
    dsgn, linvT, opbuf, colneg, total, stride = (int(v) for v in call(4, [nblk])[0])
    assert stride == NOPV * 64
    assert dsgn == 0
    assert linvT == nblk * NB                                   # kept_factor, trailing_marginals; ld of ba_hip_tile_solve
    assert opbuf == nblk * NB + nblk * NB * NB                  # both solves
    assert colneg == nblk * NB + nblk * NB * NB + nblk * NOPV * 64
    assert total == nblk * NB + nblk * NB * NB + nblk * NOPV * 64 + (nblk + 1) // 2   # nblk ints in whole doubles
    assert (total - colneg) * 8 >= nblk * 4


# ---- 4. the key of the cached distributed plan ---------------------------------------------------------------------
def plan_key(version=7, kout=8, pat=1, dense_scatter=0, layout=None):
    return int(call(5, [version, kout, pat, dense_scatter], [layout], n_out=1)[0, 0]) & (2 ** 64 - 1)


def test_plan_key_equal_inputs_equal_keys():
    assert plan_key() == plan_key()
    assert plan_key(layout="grid", dense_scatter=1) == plan_key(layout="grid", dense_scatter=1)
    assert plan_key(layout=None) == plan_key(layout="auto") == plan_key(layout="")   # build_own_map: unset = auto


def test_plan_key_tells_layouts_apart():
    """the old key ((pat ? version : 0) * 1024 + kout * 4 + pat) was the same for tri and grid"""
    keys = [plan_key(layout=lay) for lay in (None, "tri", "grid", "col", "row")]
    assert len(set(keys)) == 5
    assert plan_key(version=3, kout=16, pat=1, layout="tri") != plan_key(version=3, kout=16, pat=1, layout="grid")
    assert plan_key(pat=0, layout="tri") != plan_key(pat=0, layout="grid")


def test_plan_key_tells_exchanges_apart():
    assert plan_key(dense_scatter=0) != plan_key(dense_scatter=1)
    assert plan_key(layout="row", dense_scatter=0) != plan_key(layout="row", dense_scatter=1)


def test_plan_key_keeps_what_it_had():
    """pattern version (only with a pattern), panel width and pat still tell plans apart; no key is the `none` value"""
    keys = {plan_key(version=v, kout=k, pat=p, dense_scatter=d, layout=lay)
            for v in (0, 1, 2, 1000) for k in (3, 4, 8, 16) for p in (1,) for d in (0, 1)
            for lay in (None, "tri", "grid", "col", "row")}
    assert len(keys) == 4 * 4 * 2 * 5
    assert plan_key(version=1, pat=0) == plan_key(version=2, pat=0) != plan_key(version=2, pat=1)
    assert 2 ** 64 - 1 not in keys
