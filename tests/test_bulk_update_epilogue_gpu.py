"""The C epilogue of the bulk trailing update k_update128 (k_chol.hip): memory-side FP64 adds against read-modify-write.

By default a 128x128 block ends with `C += -acc` as no-return global FP64 atomic adds; BA_HIP_C_RMW=1 selects the
earlier epilogue, which loads C, subtracts and stores.  A tile of the trailing matrix is touched by one workgroup
per launch and fl(c + (-a)) is fl(c - a), so the two forms must give the same bits: that is what this file checks,
on the launches that reach every variant of the epilogue.

Cases (BA_HIP_KOUT = 16, BA_HIP_BULK_FULL_M = 16, so the 128-block triangle and rectangle launches run at these
sizes):
  * the seven cases of test_bulk_update_schedule_gpu.py: 48 - 54 tiles, band-edge masks of 1, 2, 8 and 16 columns
    (blocks whose K loop is skipped, so the epilogue follows the peeled column at once), diagonal blocks (masked
    adds, wave 1 returns early), two tile rows with different column sets, an odd last tile row (64-tiles beside
    the 128-blocks); `trailing`: negative pivots outside the K range; `negpanel`: every block goes through the
    64-tile fallback, which stays on plain read-modify-write in both modes;
  * dense96: 96 tiles, every tile present.  Bulk launches at a_end = 32, 48, 64 and 80 and the rectangles between
    them add into the same tiles up to four times in succession, across the two streams: an add that were still in
    flight when the next launch reads or adds to its tile would show here.

Every GPU case runs two child processes (the switch is read once per process), each with its own time limit; a
child that ends on a signal or its limit fails the test and is not run again.  Pass condition: x, the factor
storage, linvT and dsgn (and the pattern) are bitwise equal between two identical calls and between the two
epilogues, and the componentwise backward-error ratios of tile_factor_cases.check_factor are below 1 (evaluated
on the default epilogue's arrays; the other child's are the same bits).  The CPU
tests show that a plain float64 reference meets those bounds on dense96 (test_bulk_update_schedule_gpu.py shows it
for the other cases) and that c + (-a) and c - a agree bitwise in float64.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import test_bulk_update_schedule_gpu as sched  # noqa: E402
import tile_factor_cases as tf  # noqa: E402

DENSE_NT = 96
CASES = list(sched.CASES) + ["dense96"]
ARRAYS = ("x", "nzL", "storage", "linvT", "dsgn")


def build(name):
    if name != "dense96":
        return sched.build(name)
    nt, n = DENSE_NT, 64 * DENSE_NT - 11
    pairs = [(i, j, "d") for i in range(nt) for j in range(i)]
    return tf.make_case(nt, n, pairs, (), False, 4300, None, "bulk-epilogue dense96")


def test_dense96_reaches_four_bulk_launches():
    """Panels of 16: the bulk launches that take the 128-path (16 trailing tile rows or more) start at 32 .. 80."""
    a_ends = [j + 2 * sched.PANEL for j in range(0, DENSE_NT, sched.PANEL) if DENSE_NT - (j + 2 * sched.PANEL) >= 16]
    assert a_ends == [32, 48, 64, 80]


def test_reference_meets_the_bounds_dense96():
    """Soundness gate: a plain float64 reference passes check_factor on the new case."""
    c = build("dense96")
    assert c.nzL.sum() == DENSE_NT * (DENSE_NT + 1) // 2
    rf, rs = tf.check_factor(c, *tf.reference_ldlt(c))
    print("%s: reference factor ratio %.3g, solve ratio %.3g" % (c.name, rf, rs))
    assert rf < 1.0 and rs < 1.0


def test_adding_the_negation_is_subtracting():
    """fl(c + (-a)) and fl(c - a) are the same float64, signed zeros, subnormals and infinities included."""
    tiny, mn, mx = np.finfo(np.float64).smallest_subnormal, np.finfo(np.float64).tiny, np.finfo(np.float64).max
    sp = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, mn, -mn, 1.5 * mn, 0.5 * mn, 1e-310, 1.0, -1.0, 1.0 + 2.0 ** -52,
                   mx, -mx, np.inf, -np.inf])
    rng = np.random.default_rng(11)
    r1 = np.ldexp(rng.standard_normal(20000), rng.integers(-1070, 1020, 20000))
    r2 = np.ldexp(rng.standard_normal(20000), rng.integers(-1070, 1020, 20000))
    near = r1 * (1.0 + rng.integers(-4, 5, 20000) * 2.0 ** -52)   # heavy cancellation
    c = np.concatenate([np.repeat(sp, sp.size), r1, r1, rng.standard_normal(20000)])
    a = np.concatenate([np.tile(sp, sp.size), r2, near, rng.standard_normal(20000)])
    with np.errstate(invalid="ignore", over="ignore"):
        p, q = c + (-a), c - a
    nan = np.isnan(q)
    assert np.array_equal(np.isnan(p), nan) and nan.sum() == 2          # inf - inf, -inf + inf
    assert np.array_equal(p[~nan].view(np.uint64), q[~nan].view(np.uint64))
    sub = (np.abs(q) < mn) & (q != 0)
    assert sub.sum() > 100 and (q == 0).sum() > 10 and np.signbit(q[q == 0]).any()   # the edge cases are present


def test_the_switch_is_parsed_as_a_process_switch():
    """Operation 7 of ba_hostcheck_chol_launch: BA_HIP_C_RMW set (any value) / unset."""
    import ctypes
    from helpers import hostcheck_lib
    hc = hostcheck_lib()
    hc.ba_hostcheck_chol_launch.restype = ctypes.c_int
    for val, want in ((None, 0), (b"1", 1), (b"", 1)):
        s = (ctypes.c_char_p * 1)(val)
        z = np.zeros(1, dtype=np.int64)
        out = np.full(1, -1, dtype=np.int64)
        rc = hc.ba_hostcheck_chol_launch(7, 1, z.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), s,
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        assert rc == 0 and out[0] == want


def run_case(name, check):
    """Child process: the device factor of one case, twice; prints a digest per array.  `check`: also the bounds (the
    second child's arrays are compared with the first's bit for bit, which carries the bounds over)."""
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
        for what, p, q in zip(ARRAYS, outs[0], outs[1]):
            assert p.tobytes() == q.tobytes(), "%s: %s differs between two identical calls" % (c.name, what)
        rf, rs = tf.check_factor(c, *outs[0]) if check else (0.0, 0.0)
    finally:
        eng.close()
    for what, p in zip(ARRAYS, outs[0]):
        print("DIGEST %s %s" % (what, hashlib.sha256(np.ascontiguousarray(p).tobytes()).hexdigest()))
    if check:
        print("RATIO %s: factor %.3g solve %.3g" % (name, rf, rs))
    assert rf < 1.0 and rs < 1.0
    print("CASE-OK " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_epilogues_agree(name):
    base = dict(os.environ, BA_HIP_BULK_FULL_M="16", BA_HIP_KOUT="16")
    for k in ("BA_HIP_LEFT_MIN_TILES", "BA_HIP_SQUARE", "BA_HIP_SQ_W", "BA_HIP_NO128", "BA_HIP_NO_LOOKAHEAD",
              "BA_HIP_BULK_FULL", "BA_HIP_C_RMW"):
        base.pop(k, None)
    digests = {}
    for mode in ("add", "rmw"):
        env = dict(base, BA_HIP_C_RMW="1") if mode == "rmw" else base
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name, mode], env=env, capture_output=True, text=True,
                           timeout=180)
        print("\n".join(mode + " " + l for l in r.stdout.splitlines() if l.startswith("RATIO")))
        assert r.returncode == 0, mode + ": " + r.stdout[-3000:] + r.stderr[-3000:]
        assert "CASE-OK " + name in r.stdout, mode + ": " + r.stdout[-2000:]
        digests[mode] = dict(l.split()[1:3] for l in r.stdout.splitlines() if l.startswith("DIGEST"))
        assert sorted(digests[mode]) == sorted(ARRAYS)
    for what in ARRAYS:
        assert digests["add"][what] == digests["rmw"][what], "%s: %s differs between the two epilogues" % (name, what)


if __name__ == "__main__":
    run_case(sys.argv[1], sys.argv[2] == "add")
