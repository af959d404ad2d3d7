"""Marginalisation plan and dense prior error state (ba_amd/csrc/marg.h), checked on the CPU through
libba_hostcheck.so: on random small graphs the plan's blanket and counts equal a Python restatement of the
absorbed / dropped rules of ba_hip.h, every refusal fires, and the prior's d(x) and J_d agree with central
differences."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ba_amd", "lib", "libba_hostcheck.so")
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    if not hasattr(lib, "ba_hostcheck_marg_plan"):
        import __graft_entry__
        __graft_entry__.build()
        lib = ctypes.CDLL(LIB)
    lib.ba_hostcheck_marg_plan.restype = ctypes.c_int
    return lib


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1) if len(a) else np.zeros(1, np.uint32))


class Graph:
    pass


def random_graph(rng, LM, P=12, L=20):
    g = Graph()
    g.LM, g.P, g.L = LM, P, (L if LM else 0)
    g.pose_active = (rng.random(P) > 0.15).astype(np.uint8)
    g.lm_active = (rng.random(g.L) > 0.1).astype(np.uint8)
    g.lm_ref = rng.integers(0, P, g.L).astype(np.uint32)
    pp, pl = [], []
    for l in range(g.L):
        for p in rng.choice(P, size=rng.integers(2, 5), replace=False):
            pp.append(p); pl.append(l)
        if LM == 1 and rng.random() < 0.5:
            pp.append(g.lm_ref[l]); pl.append(l)  # an observation from the reference pose (no pose blocks)
    g.proj_pose, g.proj_lm = np.array(pp, np.uint32), np.array(pl, np.uint32)
    g.un = rng.integers(0, P, 4).astype(np.uint32)
    g.b1 = np.arange(0, P - 1, 2, dtype=np.uint32)
    g.b2 = g.b1 + 1
    g.i1 = np.arange(1, P - 1, 3, dtype=np.uint32)
    g.i2 = g.i1 + 1
    g.prior_ptr = np.array([0, 3, 5], np.uint32)
    g.prior_pose = np.array([2, 5, 7, 9, 10], np.uint32)
    return g


def plan(hc, g, M, Lids, D=6):
    counts = np.zeros(7, np.uint32)
    blanket = np.zeros(g.P + 1, np.uint32)
    err = ctypes.create_string_buffer(512)
    arr = [_u32(x) for x in (g.lm_ref, g.proj_pose, g.proj_lm, g.un, g.b1, g.b2, g.i1, g.i2, g.prior_ptr,
                             g.prior_pose, M, Lids)]
    pa = np.ascontiguousarray(g.pose_active)
    la = np.ascontiguousarray(g.lm_active if g.L else np.zeros(1, np.uint8))
    rc = hc.ba_hostcheck_marg_plan(
        g.LM, D, g.P, pa.ctypes.data_as(u8p), g.L, la.ctypes.data_as(u8p), arr[0].ctypes.data_as(u32p),
        len(g.proj_pose), arr[1].ctypes.data_as(u32p), arr[2].ctypes.data_as(u32p), len(g.un), arr[3].ctypes.data_as(u32p),
        len(g.b1), arr[4].ctypes.data_as(u32p), arr[5].ctypes.data_as(u32p), len(g.i1), arr[6].ctypes.data_as(u32p),
        arr[7].ctypes.data_as(u32p), len(g.prior_ptr) - 1, arr[8].ctypes.data_as(u32p), arr[9].ctypes.data_as(u32p),
        len(M), arr[10].ctypes.data_as(u32p), len(Lids), arr[11].ctypes.data_as(u32p),
        counts.ctypes.data_as(u32p), blanket.ctypes.data_as(u32p), err, 512)
    if rc != 0:
        return None, err.value.decode()
    return (counts, blanket[:counts[0]]), ""


def restate(g, M, Lids):
    """ba_hip.h: absorbed, dropped and blanket sets in plain Python"""
    M, Ls = set(int(x) for x in M), set(int(x) for x in Lids)
    act = lambda p: bool(g.pose_active[p])
    B = set()
    touch = lambda p: B.add(int(p)) if act(p) and int(p) not in M else None
    n_proj = n_drop = 0
    for p, l in zip(g.proj_pose, g.proj_lm):
        if not g.lm_active[l]:
            continue
        if int(l) in Ls:
            n_proj += 1
            if g.LM == 1 and p == g.lm_ref[l]:
                continue
            touch(p)
            if g.LM == 1:
                touch(g.lm_ref[l])
        elif int(p) in M:
            n_drop += 1
    n_un = sum(int(p) in M for p in g.un)
    n_bin = n_imu = 0
    for a, b in zip(g.b1, g.b2):
        if int(a) in M or int(b) in M:
            n_bin += 1; touch(a); touch(b)
    for a, b in zip(g.i1, g.i2):
        if int(a) in M or int(b) in M:
            n_imu += 1; touch(a); touch(b)
    n_pr = 0
    for q in range(len(g.prior_ptr) - 1):
        ps = g.prior_pose[g.prior_ptr[q]:g.prior_ptr[q + 1]]
        if any(int(p) in M for p in ps):
            n_pr += 1
            for p in ps:
                touch(p)
    return [len(B), n_proj, n_un, n_bin, n_imu, n_pr, n_drop], sorted(B)


@pytest.mark.parametrize("LM", [0, 1, 3])
def test_plan_sets_and_counts_match_restatement(hc, LM):
    rng = np.random.default_rng(10 + LM)
    checked = 0
    for trial in range(60):
        g = random_graph(rng, LM)
        act = np.flatnonzero(g.pose_active)
        M = rng.choice(act, size=min(len(act), rng.integers(1, 3)), replace=False)
        if LM == 0:
            Lids = []
        else:
            obs_by_M = set(int(l) for p, l in zip(g.proj_pose, g.proj_lm) if int(p) in set(M.tolist()))
            anchored = set(int(l) for l in range(g.L) if int(g.lm_ref[l]) in set(M.tolist()))
            cand = sorted(l for l in (obs_by_M | anchored) if g.lm_active[l])
            keep = [l for l in cand if l in anchored or (LM == 3 and rng.random() < 0.6) or (LM == 1 and rng.random() < 0.6)]
            Lids = keep
        got, err = plan(hc, g, M, Lids)
        assert got is not None, err
        want_counts, want_B = restate(g, M, Lids)
        assert got[0].tolist() == want_counts
        assert got[1].tolist() == want_B
        checked += 1
    assert checked == 60


@pytest.mark.parametrize("LM", [0, 1, 3])
def test_plan_refusals(hc, LM):
    rng = np.random.default_rng(3)
    g = random_graph(rng, LM)
    g.pose_active[:] = 1
    if g.L:
        g.lm_active[:] = 1
    g.pose_active[11] = 0
    anchored0 = [l for l in range(g.L) if g.lm_ref[l] == 0]
    ok_L = anchored0
    cases = [([], ok_L, "empty"), ([0, 0], ok_L, "twice"), ([99], ok_L, "does not exist"), ([11], [], "inactive")]
    for M, Lids, msg in cases:
        got, err = plan(hc, g, M, Lids)
        assert got is None and msg in err, (M, err)
    got, err = plan(hc, g, list(range(0, 11)), [l for l in range(g.L)], D=15)  # |M| D = 165 > 128
    assert got is None and "exceeds" in err
    if LM == 0:
        got, err = plan(hc, g, [0], [0])
        assert got is None and "LmSize 0" in err
        return
    for Lids, msg in (([999], "does not exist"), ([ok_L[0], ok_L[0]] if ok_L else [1, 1], "twice")):
        got, err = plan(hc, g, [0], Lids)
        assert got is None and msg in err, err
    g.lm_active[1] = 0
    got, err = plan(hc, g, [0], ok_L + [1])
    assert got is None and "inactive" in err
    g.lm_active[1] = 1
    if LM == 1 and ok_L:
        got, err = plan(hc, g, [0], ok_L[1:])
        assert got is None and "anchored" in err
    # the blanket limit: |B| * D > 4096 needs more poses than this graph has; a graph of 700 poses chained by
    # binary residuals into pose 0 does it
    big = Graph()
    big.LM, big.P, big.L = 0, 700, 0
    big.pose_active = np.ones(700, np.uint8)
    big.lm_active = np.zeros(0, np.uint8)
    big.lm_ref = big.proj_pose = big.proj_lm = big.un = big.i1 = big.i2 = np.zeros(0, np.uint32)
    big.b1 = np.zeros(699, np.uint32)
    big.b2 = np.arange(1, 700, dtype=np.uint32)
    big.prior_ptr = np.zeros(1, np.uint32)
    big.prior_pose = np.zeros(0, np.uint32)
    got, err = plan(hc, big, [0], [])
    assert got is None and "blanket" in err


def _random_state(rng):
    t = rng.normal(size=3)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.concatenate([t, q, rng.normal(size=3), 0.1 * rng.normal(size=6)])


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _so3_exp(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.array([0.5 * w[0], 0.5 * w[1], 0.5 * w[2], 1.0])
    return np.concatenate([np.sin(th / 2) / th * w, [np.cos(th / 2)]])


def _apply(x, delta, D):
    """ApplyUpdate (k_apply_poses): x [+] (-delta)"""
    y = x.copy()
    y[:3] -= delta[:3]
    q = _quat_mul(x[3:7], _so3_exp(-delta[3:6]))
    y[3:7] = q / np.linalg.norm(q)
    if D >= 9:
        y[7:10] -= delta[6:9]
    if D >= 15:
        y[10:16] -= delta[9:15]
    return y


def _delta(hc, x0, x, D):
    d = np.zeros(D)
    J = np.zeros((D, D))
    hc.ba_hostcheck_prior_delta(np.ascontiguousarray(x0).ctypes.data_as(dp), np.ascontiguousarray(x).ctypes.data_as(dp),
                                D, d.ctypes.data_as(dp), J.ctypes.data_as(dp))
    return d, J


@pytest.mark.parametrize("D", [6, 9, 15])
def test_prior_delta_and_jacobian(hc, D):
    rng = np.random.default_rng(D)
    for trial in range(10):
        x0 = _random_state(rng)
        d0, J0 = _delta(hc, x0, x0, D)
        assert np.abs(d0).max() < 1e-15
        assert np.array_equal(J0, np.eye(D))
        # d is the delta that takes x0 to x: applying it to x0 gives x back
        delta = 0.3 * rng.normal(size=D)
        x = _apply(x0, delta, D)
        d, J = _delta(hc, x0, x, D)
        np.testing.assert_allclose(d, delta, rtol=1e-12, atol=1e-12)
        # J_d = dd(x [+] (-e)) / de at e = 0, central differences
        h = 1e-5
        Jfd = np.zeros((D, D))
        for k in range(D):
            e = np.zeros(D)
            e[k] = h
            Jfd[:, k] = (_delta(hc, x0, _apply(x, e, D), D)[0] - _delta(hc, x0, _apply(x, -e, D), D)[0]) / (2 * h)
        assert np.abs(Jfd - J).max() <= 1e-7 * max(1.0, np.abs(J).max())
