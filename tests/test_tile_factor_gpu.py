"""The device tile-sparse L D L^T factor (k_chol.hip) on explicit tile patterns, through Engine.tile_solve: the
grid of tile_factor_cases.py under every kernel variant, checked against the componentwise backward-error
bounds in long double (pass condition: ratio < 1; test_tile_factor.py shows on the CPU that a plain reference
passes them and subtly wrong factors do not).  Worst ratios measured on the MI355X: DESIGN.md section 8.

In-process variants (environment read on every call): BA_HIP_KOUT, BA_HIP_LEFT_MIN_TILES, BA_HIP_SQUARE /
BA_HIP_SQ_W.  Per-process switches (read once): a child pytest process re-runs a core subset of this grid."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tile_factor_cases as tf
from ba_amd import hipapi, scene

pytestmark = pytest.mark.gpu

NESTED = bool(os.environ.get("BA_TEST_NESTED"))
MANAGED = ("BA_HIP_KOUT", "BA_HIP_LEFT_MIN_TILES", "BA_HIP_SQUARE", "BA_HIP_SQ_W")
VARIANTS = {
    "default": {},
    "kout3": {"BA_HIP_KOUT": "3"},      # ragged sub-panels (KIN = 4 > 3), odd panel starts: no 128-path on the chain
    "kout8": {"BA_HIP_KOUT": "8"},      # two sub-panels of 4 per outer panel
    "kout16": {"BA_HIP_KOUT": "16"},    # four sub-panels of 4
    "left4": {"BA_HIP_LEFT_MIN_TILES": "1", "BA_HIP_KOUT": "4"},    # left-looking, the sub-panel of 8 cut at 4
    "left16": {"BA_HIP_LEFT_MIN_TILES": "1", "BA_HIP_KOUT": "16"},  # left-looking, two sub-panels of 8
    "square1": {"BA_HIP_SQUARE": "1", "BA_HIP_SQ_W": "1"},
    "square2": {"BA_HIP_SQUARE": "1", "BA_HIP_SQ_W": "2"},
    "square3": {"BA_HIP_SQUARE": "1", "BA_HIP_SQ_W": "3"},
    "square4": {"BA_HIP_SQUARE": "1", "BA_HIP_SQ_W": "4"},
}
# the child processes of test_per_process_switch: these families at these tile counts, KOUT unset and 16
CORE_FAMILIES = ("lone1", "lone2", "reverse_arrow", "blockdiag", "random_a", "dense")
CORE_SIZES = (24, 25, 48, 49)

_cases = {}


def case(family, nt, n, sign, graded):
    key = (family, nt, n, sign, graded)
    if key not in _cases:
        _cases[key] = tf.family_case(family, nt, n, sign, graded)
    return _cases[key]


@pytest.fixture(scope="module")
def eng():
    e = hipapi.Engine(1, 6)
    yield e
    e.close()


def set_variant(monkeypatch, variant):
    for k in MANAGED:
        if k in VARIANTS[variant]:
            monkeypatch.setenv(k, VARIANTS[variant][k])
        elif not NESTED:  # (a child process keeps what its parent set for the whole process)
            monkeypatch.delenv(k, raising=False)


def solve_and_check(eng, c, explicit_map):
    a = tf.lower_dense(c)
    tmap = c.tile_map if explicit_map else None
    x, rc, nzL, st, linvT, dsgn = eng.tile_solve(a, c.b, tmap, keep_factor=True)
    assert rc == 0, c.name
    x2, rc2, nzL2, st2, linvT2, dsgn2 = eng.tile_solve(a, c.b, tmap, keep_factor=True)
    assert rc2 == 0
    for name, p, q in (("x", x, x2), ("storage", st, st2), ("linvT", linvT, linvT2), ("dsgn", dsgn, dsgn2), ("nzL", nzL, nzL2)):
        assert p.tobytes() == q.tobytes(), "%s: %s differs between two identical calls" % (c.name, name)
    return tf.check_factor(c, x, nzL, st, linvT, dsgn)


def family_combos(family):
    if not NESTED:
        return tf.combos(family)
    if family == "dense":  # the trailing-half-negative dense case
        return [(nt, n, "trailing", False) for nt, n in tf.SIZES if nt in CORE_SIZES]
    return tf.combos(family, CORE_SIZES)


@pytest.mark.parametrize("family", tf.FAMILIES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_grid(eng, monkeypatch, variant, family):
    set_variant(monkeypatch, variant)
    worst = {}  # per size class (up to 5 tiles / from 24 tiles): [factor ratio, solve ratio]
    for nt, n, sign, graded in family_combos(family):
        c = case(family, nt, n, sign, graded)
        # the declared-superset family needs its map; of the others, the even tile counts derive it from the nonzeros
        rf, rs = solve_and_check(eng, c, family == "superset" or nt % 2 == 1)
        w = worst.setdefault("small" if nt <= tf.SMALL_NT else "large", [0.0, 0.0])
        w[0], w[1] = max(w[0], rf), max(w[1], rs)
    for k, w in sorted(worst.items()):
        print("RATIO %s %s %s: factor %.3g solve %.3g" % (variant, family, k, w[0], w[1]))


PROCESS_SWITCHES = {
    "bulk_full_m16": {"BA_HIP_BULK_FULL_M": "16"},     # k_update128 from 16 trailing tile rows on
    "no128": {"BA_HIP_NO128": "1"},                    # the 64-tile kernels everywhere
    "no_lookahead": {"BA_HIP_NO_LOOKAHEAD": "1"},      # one stream
    "bulk_full": {"BA_HIP_BULK_FULL": "1"},            # the uncapped bulk update
    "bulk_full_m16_left": {"BA_HIP_BULK_FULL_M": "16", "BA_HIP_LEFT_MIN_TILES": "1"},
}


@pytest.mark.parametrize("switch", list(PROCESS_SWITCHES))
def test_per_process_switch(switch):
    """The switches k_chol.hip reads once per process: a fresh child process (one at a time) runs the core
    subset of the grid with the switch set.  A child that ends on a signal or its time limit fails the test."""
    if NESTED:
        pytest.skip("nested run")
    env = dict(os.environ, BA_TEST_NESTED="1", **PROCESS_SWITCHES[switch])
    for k in MANAGED:
        if k not in PROCESS_SWITCHES[switch]:
            env.pop(k, None)
    sel = "test_grid and (default or kout16) and (%s)" % " or ".join(CORE_FAMILIES)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=300)
    print("\n".join(l[l.index("RATIO"):].replace("RATIO", "RATIO " + switch) for l in r.stdout.splitlines() if "RATIO" in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "%d passed" % (2 * len(CORE_FAMILIES)) in r.stdout, r.stdout[-2000:]


# ---- breakdown and refusals ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "kout16", "square4"])
def test_singular_pivot_and_nan_are_reported(eng, monkeypatch, variant):
    set_variant(monkeypatch, variant)
    c = case("blockdiag", 33, 2095, "spd", False)
    good = tf.lower_dense(c)
    r = 64 * 17 + 5
    a = good.copy()
    a[r, :] = 0.0   # row and column r empty, diagonal included: the pivot of row r is exactly zero
    a[:, r] = 0.0
    _, rc, _ = eng.tile_solve(a, c.b, c.tile_map)
    assert rc == 4  # ba::FactorizationError
    a = good.copy()
    assert c.tile_map[17, 16]
    a[64 * 17 + 3, 64 * 16 + 2] = np.nan
    _, rc, _ = eng.tile_solve(a, c.b, c.tile_map)
    assert rc == 4
    # the same engine solves the next case correctly
    nxt = case("blockdiag", 5, 320, "every7", False)
    solve_and_check(eng, nxt, True)
    solve_and_check(eng, c, True)


def test_refusals(eng):
    c = case("loop", 5, 320, "spd", False)
    a = tf.lower_dense(c)
    m = c.tile_map.copy()
    m[4, 0] = 0
    with pytest.raises(hipapi.HipError, match="not in the tile map"):
        eng.tile_solve(a, c.b, m)
    with pytest.raises(hipapi.HipError, match="NULL or empty"):
        eng.tile_solve(np.zeros((0, 0)), np.zeros(0))
    x = np.zeros(320)
    dp = hipapi.dp
    for args in ((None, c.b.ctypes.data_as(dp), x.ctypes.data_as(dp)), (a.ctypes.data_as(dp), None, x.ctypes.data_as(dp)),
                 (a.ctypes.data_as(dp), c.b.ctypes.data_as(dp), None)):
        rc = eng.L.ba_hip_tile_solve(eng.h, 320, args[0], args[1], None, args[2], None, None, None, None)
        assert rc < 0
        assert b"NULL or empty" in eng.L.ba_hip_last_error(eng.h)
    # and the engine still works
    solve_and_check(eng, c, True)


def test_engine_with_a_scene_is_left_alone():
    """solve_gn gives the same bits before and after a tile_solve; the marginals never read the foreign factor."""
    from test_marginals_gpu import _engine
    sc = scene.make_scene(70, 300, 6, lm_dim=1, seed=14)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _engine(sc, 1, pa, tvs=True)
    e = s.eng
    e.linearize()
    assert e.solve_gn() == 0
    before = [np.array(v) for v in e.get_delta_gn()]
    cov = e.pose_marginals([1, 2])
    cal = e.get_calibration_marginals()
    joint = e.joint_marginals([1, 2])
    c = case("reverse_arrow", 5, 320, "every7", False)
    solve_and_check(e, c, True)
    # the selected inverse computed before the foreign solve is still the scene's
    assert np.array_equal(e.pose_marginals([1, 2]), cov)
    # what would have to read the kept factor again is refused
    with pytest.raises(hipapi.HipError, match="replaced the kept factor"):
        e.get_calibration_marginals()
    with pytest.raises(hipapi.HipError, match="replaced the kept factor"):
        e.joint_marginals([1, 2])
    e.linearize()  # (drops the selected inverse)
    with pytest.raises(hipapi.HipError):
        e.compute_marginals()
    assert e.solve_gn() == 0
    for p, q in zip(before, e.get_delta_gn()):
        assert np.array_equal(p, q)
    assert np.array_equal(e.pose_marginals([1, 2]), cov)
    assert np.array_equal(e.get_calibration_marginals(), cal)
    assert np.array_equal(e.joint_marginals([1, 2]), joint)
    # directly after a tile_solve with no selected inverse at hand: refused
    solve_and_check(e, c, True)
    e.linearize()
    assert e.solve_gn() == 0
    solve_and_check(e, c, True)
    with pytest.raises(hipapi.HipError, match="replaced the kept factor"):
        e.compute_marginals()
    e.close()
