"""Leverages of unary, binary and inertial residuals on the CPU: pose_pose_leverage_host (ba_amd/csrc/pplever.h, the
plain C++ restatement of k_pplever.hip's formula and index logic, through ba_hostcheck_pose_pose_leverages) against
a reference that uses no inverse — the diagonal blocks of Q Q^T for the thin QR of the dense whitened Jacobian.
Jacobians from the oracle; Lambda is the test's own (pplever_cases.informations), G its Cholesky factor; whitened
blocks G^T C G are compared absolutely with max(1e-9, 4.5 eps cond(S)) (leverage_cases.tolerance, DESIGN.md
section 8), which also rejects a scene that pushes the bound above 1e-8."""
import types

import numpy as np
import pytest

from ba_amd import scene
from helpers import accepted_obs, fill, gn_options, hostcheck_lib
import leverage_cases as lc
import pplever_cases as pc

_cache = {}


def _finish(c):
    """dense references and the host result of a case: computed once, shared, read only"""
    t, D, pa, masks = c["t"], c["D"], c["pa"], c["masks"]
    c["lam"] = c["info"] * c["w"][:, None, None]
    Jpp, off, G = pc.whitened_rows(t, D, c["dz"], c["lam"], pa, masks)
    n = Jpp.shape[1]
    if "Jproj" in c:
        J = np.vstack([c["Jproj"], np.hstack([Jpp, np.zeros((Jpp.shape[0], c["Jproj"].shape[1] - n))])])
        row0 = c["Jproj"].shape[0]
    else:
        J, row0 = Jpp, 0
    H = J.T @ J   # landmarks eliminated as leverage_cases.reduced_system does; masked parameters as the engine
    S = H[:n, :n] - H[:n, n:] @ np.linalg.solve(H[n:, n:], H[n:, :n]) if H.shape[0] > n else H
    S = pc.masked_diagonal(S, pa, masks, D)
    c.update(J=J, off=off, G=G, n=n, S=S, sigma=np.linalg.inv(S), R=pc.res_dim(t, D))
    c["tol"] = lc.tolerance(S)
    c["want"] = pc.qr_blocks(J, row0, off)
    c["cov"], c["lam_host"], c["lev"] = _host(c, 0)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _host(c, variant):
    return pc.host_leverages(hostcheck_lib(), c["t"], c["D"], c["dz"], c["info"], c["w"], c["pa"], c["masks"],
                             c["sigma"], variant)


def _graph(po):
    if "graph" not in _cache:
        sc, t, pa, masks = pc.pose_graph()
        ba = po.OracleBundleAdjuster(0, 6)
        ba.Init(gn_options(po, apply_results=0))
        ba.add_poses(sc.poses, is_active=pa)
        pc.add_to_oracle(ba, sc, t)
        ba.Solve(1)
        dz, _ = pc.oracle_jacobians(ba, t)
        info, w = pc.informations(t)
        _cache["graph"] = _finish(dict(t=t, D=6, pa=pa, masks=masks, dz=dz, info=info, w=w))
    return _cache["graph"]


def _mixed(po):
    if "mixed" not in _cache:
        sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
        pa = np.ones(sc.num_poses, dtype=np.uint8)
        pa[sc.anchor_poses] = 0
        la = np.ones(sc.num_landmarks, dtype=np.uint8)
        t = pc.helper_terms(sc, sc.num_poses)
        ba = po.OracleBundleAdjuster(1, 6)
        ba.Init(gn_options(po, apply_results=0))
        fill(ba, sc, active=pa)
        pc.add_to_oracle(ba, sc, t)
        ba.Solve(1)
        jm, jr, jl = ba.proj_jacobians()
        pw = ba.proj_weights()
        acc = np.array(accepted_obs(sc), dtype=np.int64)
        pp, pl = acc[:, 0], acc[:, 2]
        sw = np.sqrt(pw)[:, None, None]
        Jproj, n = lc.dense_jacobian(1, 6, 0, pa, la, sc.lm_ref_pose, pp, pl, sw * jm, sw * jr, sw * jl)
        dz, _ = pc.oracle_jacobians(ba, t)
        info, w = pc.informations(t)
        masks = np.zeros(sc.num_poses, np.uint16)
        c = _finish(dict(t=t, D=6, pa=pa, masks=masks, dz=dz, info=info, w=w, Jproj=Jproj))
        assert c["n"] == n
        c["proj"] = lc.host_leverages(hostcheck_lib(), 1, 6, 0, pa, la, sc.lm_ref_pose, pp, pl, jm, jr, jl, None, pw,
                                      c["sigma"])
        c["setup"] = types.SimpleNamespace(masks=masks, pa=pa, obs_lm=pl, la=la, D=6, K=0, lm_dim=1)
        _cache["mixed"] = c
    return _cache["mixed"]


def _imu(po):
    if "imu" not in _cache:
        sc, t, pa, masks = pc.imu_window()
        o = pc.widen_imu_noise(gn_options(po, apply_results=0, use_robust_norm_for_inertial_residuals=0))
        ba = po.OracleBundleAdjuster(0, 15)
        ba.Init(o)
        ba.SetGravity(sc.gravity)
        ba.add_poses(sc.poses, v_w=sc.init_vel, b=sc.init_bias, is_active=pa, time=sc.pose_time)
        pc.add_to_oracle(ba, sc, t)
        ba.Solve(1)
        dz, ci = pc.oracle_jacobians(ba, t)
        info, w = pc.informations(t, imu_cov_inv=ci)
        _cache["imu"] = _finish(dict(t=t, D=15, pa=pa, masks=masks, dz=dz, info=info, w=w))
    return _cache["imu"]


CASES = {"graph": _graph, "mixed": _mixed, "imu": _imu}


@pytest.mark.parametrize("name", ["graph", "mixed", "imu"])
def test_host_formula_equals_qr_blocks(oracle_lib, name):
    c = CASES[name](oracle_lib)
    got = pc.whiten(c["cov"], c["G"], c["R"])
    err = pc.block_err(got, c["want"])
    print("%s: max |G^T C G - QQ^T blocks| = %.3g over %d residuals, tol %.3g, cond(S) %.3g" %
          (name, err, len(got), c["tol"], np.linalg.cond(c["S"])))
    assert err <= c["tol"]
    assert np.array_equal(c["cov"], np.transpose(c["cov"], (0, 2, 1)))
    lam = c["lam"]
    assert np.abs(c["lam_host"] - lam).max() <= 1e-12 * np.abs(lam).max()
    # the leverage is the trace of the whitened block
    tr = np.array([np.trace(g) for g in got])
    assert np.abs(c["lev"] - tr).max() <= c["tol"]


@pytest.mark.parametrize("name", ["graph", "mixed", "imu"])
def test_blocks_lie_between_zero_and_identity(oracle_lib, name):
    c = CASES[name](oracle_lib)
    ev = np.concatenate([np.linalg.eigvalsh(0.5 * (g + g.T)) for g in pc.whiten(c["cov"], c["G"], c["R"])])
    print("%s: eigenvalues in [%.3g, %.12g]" % (name, ev.min(), ev.max()))
    assert ev.min() >= -c["tol"] and ev.max() <= 1 + c["tol"]


@pytest.mark.parametrize("name", ["graph", "imu"])
def test_leverages_sum_to_the_unknown_count(oracle_lib, name):
    """a pure pose graph: every unmasked parameter of an active pose is an unknown that some residual touches"""
    c = CASES[name](oracle_lib)
    masked = sum(bin(int(m)).count("1") for m, a in zip(c["masks"], c["pa"]) if a)
    unknowns = int(c["pa"].sum()) * c["D"] - masked
    assert unknowns == int((np.abs(c["J"]).max(0) > 0).sum())
    total = c["lev"].sum()
    print("%s: sum of leverages %.12g, unknowns %d" % (name, total, unknowns))
    assert abs(total - unknowns) <= 1e-8 * unknowns


def test_whole_system_trace_identity(oracle_lib):
    """projection and pose-pose residuals in one system: sum tr H_proj + sum l_pp = unknowns"""
    c = _mixed(oracle_lib)
    unknowns = lc.unknowns_seen(c["setup"])
    assert unknowns == c["J"].shape[1]
    tr_proj = np.trace(c["proj"], axis1=1, axis2=2).sum()
    total = tr_proj + c["lev"].sum()
    print("sum tr H_proj %.10g + sum l_pp %.10g = %.12g, unknowns %d" % (tr_proj, c["lev"].sum(), total, unknowns))
    assert c["lev"].sum() > 1.0
    assert abs(total - unknowns) <= 1e-7 * unknowns


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_wrong_variants_are_told_apart(oracle_lib, variant):
    """1: the cross block Sigma_{p1 p2} dropped; 2: masked columns left in J; 3: the binary weight left out of
    Lambda.  Each misses the QR blocks by more than 100 x the tolerance on the pose graph."""
    c = _graph(oracle_lib)
    cov, lam, lev = _host(c, variant)
    # the whitening stays the test's own: a wrong Lambda shows in the leverage tr(C Lambda) and in the info output
    err = pc.block_err(pc.whiten(cov, c["G"], c["R"]), c["want"])
    err = max(err, np.abs(lev - np.array([np.trace(w) for w in c["want"]])).max())
    print("variant %d: max error %.3g (tolerance %.3g)" % (variant, err, c["tol"]))
    assert err > 100 * c["tol"]
