"""Leverages of unary, binary and inertial residuals on the MI355X (ba_hip_get_pose_pose_leverages, k_pplever.hip):
C = J Sigma_ee J^T, the effective information Lambda and tr(C Lambda) per residual, against J Sigma_ee J^T in numpy
(Sigma = inv(get_S()) with keep_reduced_system, Jacobians from the oracle at the linearisation state) and against the
diagonal blocks of Q Q^T of the dense whitened Jacobian.  Whitened blocks G^T C G, with G the Cholesky factor of the
TEST's Lambda (unary: cov_inv x ba_hip_get_unary_scales; binary: weight x sqrt^T sqrt; inertial: the oracle's
cov_inv), are compared absolutely with max(1e-9, 4.5 eps cond(S)) (every scene must keep it at
or below 1e-8); the call's info output is compared with that Lambda separately, to 1e-12 relative."""
import ctypes
import gc

import numpy as np
import pytest

from ba_amd import hipapi, scene
from oracle import pyoracle as po
from helpers import gn_options
import leverage_cases as lc
import pplever_cases as pc

pytestmark = pytest.mark.gpu

KINDS = (hipapi.RES_UNARY, hipapi.RES_BINARY, hipapi.RES_IMU)
CALL = "ba_hip_get_pose_pose_leverages: "


def _fixed(sc, more=2):
    """the anchors and `more` further poses inactive (as tests/test_leverages_gpu.py)"""
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    free = [p for p in range(sc.num_poses) if pa[p]]
    pa[free[len(free) // 3::len(free) // 3][:more]] = 0
    return pa


def _pose_jacobians(sc, t, D=6, options=None, pa=None):
    """dz (and the inertial cov_inv) of the pose-pose residuals from the oracle at the scene's initial state: they
    depend on the poses alone, so the oracle gets no landmarks"""
    ba = po.OracleBundleAdjuster(0, D)
    ba.Init(gn_options(po, apply_results=0) if options is None else options)
    if D > 6:
        ba.SetGravity(sc.gravity)
        ba.add_poses(sc.poses, v_w=sc.init_vel, b=sc.init_bias, is_active=pa, time=sc.pose_time)
    else:
        ba.add_poses(sc.poses, is_active=pa)
    pc.add_to_oracle(ba, sc, t)
    ba.Solve(1)
    return pc.oracle_jacobians(ba, t)


def _unary_scales(eng, n):
    s = np.ones(max(n, 1))
    eng._chk(eng.L.ba_hip_get_unary_scales(eng.h, s.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return s[:n]


def _all_kinds(eng, t):
    """the three outputs of every residual, kinds concatenated in slot order"""
    cov, info, lev = [], [], []
    for kind in KINDS:
        if t.counts[kind]:
            c, i, l = eng.pose_pose_leverages(kind)
            assert c.shape == (t.counts[kind], 15, 15) and l.shape == (t.counts[kind],)
            cov.append(c), info.append(i), lev.append(l)
    return np.concatenate(cov), np.concatenate(info), np.concatenate(lev)


def _check(name, eng, t, D, dz, pa, masks, S, imu_cov_inv=None, qr=False):
    """every residual of every kind against the numpy reference (and the QR blocks of a pure pose graph)"""
    tol = lc.tolerance(S)
    sigma = np.linalg.inv(S)
    info, w = pc.informations(t, un_scale=_unary_scales(eng, t.counts[0]), imu_cov_inv=imu_cov_inv)
    lam = info * w[:, None, None]
    R = pc.res_dim(t, D)
    J, off, G = pc.whitened_rows(t, D, dz, lam, pa, masks)
    cov, got_info, lev = _all_kinds(eng, t)
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(lev))
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1))), "cov is not bitwise symmetric"
    for q in range(len(R)):   # zero outside the residual's own block
        assert not cov[q, R[q]:, :].any() and not cov[q, :, R[q]:].any()
        assert not got_info[q, R[q]:, :].any() and not got_info[q, :, R[q]:].any()
    e_info = max(np.abs(got_info[q] - lam[q]).max() / np.abs(lam[q]).max() for q in range(len(R)))
    got = pc.whiten(cov, G, R)
    want = pc.whiten(pc.reference_cov(t, D, dz, pa, masks, sigma), G, R)
    e_ref = pc.block_err(got, want)
    e_lev = max(abs(lev[q] - np.trace(got[q])) / R[q] for q in range(len(R)))
    ev = np.concatenate([np.linalg.eigvalsh(0.5 * (g + g.T)) for g in got])
    print("%s: |G^T C G - reference| %.3g, |l - tr| / R %.3g, info rel %.3g, tol %.3g, cond(S) %.3g, eig in [%.3g, %.12g]"
          % (name, e_ref, e_lev, e_info, tol, np.linalg.cond(S), ev.min(), ev.max()))
    assert e_info <= 1e-12
    assert e_ref <= tol and e_lev <= tol
    assert ev.min() >= -tol and ev.max() <= 1 + tol
    if qr:
        e_qr = pc.block_err(got, pc.qr_blocks(J, 0, off))
        print("%s: |G^T C G - QR blocks| %.3g" % (name, e_qr))
        assert e_qr <= tol
    return cov, got_info, lev, G, R, tol


# ---- LmSize 0: the 12-pose graph ---------------------------------------------------------------------------
def _graph_engine(mode=hipapi.ORDER_NATURAL, perm=None, finalize=True):
    sc, t, pa, masks = pc.pose_graph()
    eng = hipapi.Engine(0, 6)
    o = hipapi.Options()
    o.keep_reduced_system = 1
    eng.set_options(o)
    eng.set_cameras(np.array([[500.0, 500.0, 320.0, 240.0]]), [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    pc.add_to_engine(eng, t)
    eng.set_pose_ordering(mode)
    if perm is not None:
        eng.set_pose_permutation(perm)
    if finalize:
        eng.finalize()
        eng.begin_solve()
        eng.set_pose_masks(masks)
        eng.linearize()
        assert eng.solve_gn() == 0
    return eng, sc, t, pa, masks


_graph_dz = {}


def _graph_jacobians(sc, t, pa):
    if "dz" not in _graph_dz:
        _graph_dz["dz"] = _pose_jacobians(sc, t, pa=pa)[0]
        _graph_dz["dz"].setflags(write=False)
    return _graph_dz["dz"]


def test_pose_graph_without_landmarks():
    """LmSize 0: all three outputs of the unary and binary residuals against J Sigma_ee J^T and the QR blocks; the
    leverages sum to the unmasked active unknowns (each of the sum_i R_i diagonal entries within the tolerance)."""
    eng, sc, t, pa, masks = _graph_engine()
    dz = _graph_jacobians(sc, t, pa)
    S = eng.get_S()
    cov, info, lev, G, R, tol = _check("graph", eng, t, 6, dz, pa, masks, S, qr=True)
    unknowns = int(pa.sum()) * 6 - 3
    print("graph: sum of leverages %.12g of %d" % (lev.sum(), unknowns))
    assert abs(lev.sum() - unknowns) <= R.sum() * tol
    st = eng.pose_pose_leverage_stats()
    nb = t.counts[1]
    live = sum(int(pa[a]) + int(pa[b]) for a, b in zip(t.bin_p1, t.bin_p2))
    assert st["residuals"] == nb and st["kind"] == hipapi.RES_BINARY and st["device_ms"] > 0
    assert st["sigma_blocks"] == sum((int(pa[a]) + int(pa[b])) ** 2 for a, b in zip(t.bin_p1, t.bin_p2)) > live
    # the odometry into and out of the inactive pose keeps one D x D block; a weight scales info, not cov
    sl = t.kind_slice(hipapi.RES_BINARY)
    assert np.abs(cov[sl][4]).max() > 0 and np.abs(cov[sl][5]).max() > 0
    eng.close()


def test_binary_weight_and_translation_only():
    """weight != 1 and use_rotation = 0 (the second loop closure: weight 0.4): rows 3..5 of J are zero, so C is zero
    there and the residual has rank 3; info = weight x sqrt^T sqrt in full."""
    eng, sc, t, pa, masks = _graph_engine()
    dz = _graph_jacobians(sc, t, pa)
    k = t.counts[1] - 1
    assert t.bin_rot[k] == 0 and t.bin_w[k] == 0.4 and t.bin_w[2] == 2.5
    S = eng.get_S()
    tol = lc.tolerance(S)
    sigma = np.linalg.inv(S)
    cov, info, lev = eng.pose_pose_leverages(hipapi.RES_BINARY, [k, 2])
    lam = np.stack([t.bin_w[i] * t.bin_sqrt[i].T @ t.bin_sqrt[i] for i in (k, 2)])
    assert np.abs(info[:, :6, :6] - lam).max() <= 1e-12 * np.abs(lam).max()
    assert not cov[0, 3:, :].any() and not cov[0, :, 3:].any() and np.abs(cov[0, :3, :3]).max() > 0
    nu = t.counts[0]
    assert not dz[nu + k, :, 3:6].any()
    ref = pc.reference_cov(t, 6, dz, pa, masks, sigma)[[nu + k, nu + 2]]
    for q in range(2):
        g = np.linalg.cholesky(lam[q])
        got, want = g.T @ cov[q, :6, :6] @ g, g.T @ ref[q, :6, :6] @ g
        assert np.abs(got - want).max() <= tol
        assert abs(lev[q] - np.trace(want)) <= 6 * tol
    # (three live rows: the leverage of the translation-only closure cannot exceed 3)
    assert 1e-3 < lev[0] < 3.0 and 1e-3 < lev[1] < 6.0
    eng.close()


def test_by_id_equals_all_bitwise_and_orderings_agree():
    """Reversed ids with a repeat equal the all-residuals output bit for bit, two calls give the same bits, and
    BA_HIP_ORDER_AUTO and a reversed pose order change nothing beyond the tolerance."""
    res = []
    n_act = int(pc.pose_graph()[2].sum())
    rev = np.arange(n_act, dtype=np.uint32)[::-1]
    for mode in (hipapi.ORDER_NATURAL, hipapi.ORDER_AUTO, hipapi.ORDER_USER):
        eng, sc, t, pa, masks = _graph_engine(mode, rev if mode == hipapi.ORDER_USER else None)
        out = {}
        for kind in (hipapi.RES_UNARY, hipapi.RES_BINARY):
            every = eng.pose_pose_leverages(kind)
            again = eng.pose_pose_leverages(kind)
            n = t.counts[kind]
            ids = np.concatenate([np.arange(n)[::-1], [1, 1, 0]]).astype(np.uint32)
            per = eng.pose_pose_leverages(kind, ids)
            for a, b, c in zip(every, again, per):
                assert np.array_equal(a, b)
                assert np.array_equal(c, a[ids])
            only = eng.pose_pose_leverages(kind, ids[:2], want=(False, False, True))
            assert only[0] is None and only[1] is None and np.array_equal(only[2], every[2][ids[:2]])
            assert eng.pose_pose_leverage_stats()["residuals"] == 2
            out[kind] = every
        S = eng.get_S()
        info, w = pc.informations(t, un_scale=_unary_scales(eng, t.counts[0]))
        G = pc.whitened_rows(t, 6, _graph_jacobians(sc, t, pa), info * w[:, None, None], pa, masks)[2]
        cov = np.concatenate([out[hipapi.RES_UNARY][0], out[hipapi.RES_BINARY][0]])
        res.append((pc.whiten(cov, G, pc.res_dim(t, 6)), lc.tolerance(S)))
        eng.close()
    (nat, tol), (auto, _), (user, _) = res
    print("natural against AUTO: %.3g, against a reversed order: %.3g, tol %.3g" %
          (pc.block_err(auto, nat), pc.block_err(user, nat), tol))
    assert pc.block_err(auto, nat) <= tol and pc.block_err(user, nat) <= tol


# ---- LmSize 1: inside a visual system ----------------------------------------------------------------------
def test_visual_scene_completes_the_trace_identity():
    """make_scene(12, 60, 4) with priors, odometry and three masked parameters of the first active pose (the setup
    of test_pose_pose_terms_and_masks): the pose-pose blocks against the reference, and sum tr H_proj + sum l_pp =
    the unknowns, which the projection leverages alone miss."""
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    pa = _fixed(sc)
    masks = np.zeros(sc.num_poses, dtype=np.uint16)
    masks[int(np.nonzero(pa)[0][0])] = 0x7
    s = lc.engine(sc, 1, pa, pose_pose=True, masks=masks)
    lc.solve(s)
    t = pc.helper_terms(sc, sc.num_poses)
    dz, _ = _pose_jacobians(sc, t, pa=pa)
    S = s.eng.get_S()
    cov, info, lev, G, R, tol = _check("visual", s.eng, t, 6, dz, pa, masks, S)
    tr_proj = np.trace(s.eng.projection_leverages(), axis1=1, axis2=2).sum()
    unknowns = lc.unknowns_seen(s)
    print("visual: sum tr H_proj %.10g + sum l_pp %.10g = %.12g of %d" % (tr_proj, lev.sum(), tr_proj + lev.sum(), unknowns))
    assert lev.sum() > 0.5
    assert abs(tr_proj + lev.sum() - unknowns) <= 1e-7 * unknowns
    assert abs(tr_proj - unknowns) > 1e-3 * unknowns
    s.eng.close()


def test_pose_blocks_straddle_tiles():
    """make_scene(83, 500, 6) with pose-pose terms: 79 active poses, 474 rows, no multiple of 64 — pose blocks
    straddle the 64-tiles, so one Sigma_ee is read across tile boundaries."""
    sc = scene.make_scene(83, 500, 6, lm_dim=1, seed=11)
    pa = _fixed(sc)
    assert int(pa.sum()) == 79
    s = lc.engine(sc, 1, pa, pose_pose=True)
    lc.solve(s)
    t = pc.helper_terms(sc, sc.num_poses)
    dz, _ = _pose_jacobians(sc, t, pa=pa)
    S = s.eng.get_S()
    assert S.shape[0] == 474 and S.shape[0] % 64 != 0
    rows = pc.natural_rows(pa, 6)
    crossing = [q for q, (a, b) in enumerate(zip(t.p1, t.p2))
                if any(p != pc.NONE and rows[p] >= 0 and rows[p] // 64 != (rows[p] + 5) // 64 for p in (a, b))]
    assert crossing, "no residual with a pose block across a tile boundary"
    _check("straddle", s.eng, t, 6, dz, pa, s.masks, S)
    s.eng.close()


# ---- PoseSize 15 through the class -------------------------------------------------------------------------
def test_inertial_window_through_the_class():
    """PoseSize 15, 8 poses, inertial residuals, priors and odometry through ba::BundleAdjuster (adjuster.py ->
    ba_capi): 15 x 15 blocks with R = 15, the conditioning residual (first pose inactive) whose dz1 block drops;
    GetImuLeverage and the batched call agree with the C-ABI bit for bit."""
    from ba_amd import adjuster
    sc, t, pa, _ = pc.imu_window()
    assert pa[t.imu_p1[0]] == 0 and pa[t.imu_p2[0]] == 1, "no conditioning residual"
    D = 15

    def options(o):
        o.use_dogleg = 0
        o.error_change_threshold = 0
        o.param_change_threshold = 0
        o.use_robust_norm_for_inertial_residuals = 0
        return pc.widen_imu_noise(o)

    o = options(adjuster.default_options())
    o.write_reduced_camera_matrix = 1
    h = adjuster.BundleAdjuster(0, D)
    h.Init(o)
    h.SetGravity(sc.gravity)
    h.add_poses(sc.poses, v_w=sc.init_vel, b=sc.init_bias, is_active=pa, time=sc.pose_time)
    pc.add_to_oracle(h, sc, t)
    h.Solve(1)
    assert adjuster.RESULT_NAMES[h.summary().result] not in ("FactorizationError", "SolverError")
    eng = h.engine()
    S = eng.get_S()
    S = np.where(S == 0.0, S.T, S)   # (get_S keeps one block triangle with use_triangular_matrices)
    assert S.shape == (int(pa.sum()) * D,) * 2
    # the masks the class uploaded (regularisation) show as 1e6 on the diagonal of S
    rows = pc.natural_rows(pa, D)
    masks = np.zeros(len(pa), np.uint16)
    for p in np.nonzero(pa)[0]:
        for c in range(D):
            if S[rows[p] + c, rows[p] + c] == 1e6:
                masks[p] |= 1 << c
    oo = options(gn_options(po, apply_results=0))
    dz, ci = _pose_jacobians(sc, t, D=D, options=oo, pa=pa)
    cov, info, lev, G, R, tol = _check("inertial", eng, t, D, dz, pa, masks, S, imu_cov_inv=ci)
    sl = t.kind_slice(hipapi.RES_IMU)
    assert np.all(R[sl] == 15) and np.abs(cov[sl][:, 9:, 9:]).max() > 0
    masked = sum(bin(int(m)).count("1") for m in masks)
    unknowns = int(pa.sum()) * D - masked
    print("inertial: sum of leverages %.12g of %d (%d masked)" % (lev.sum(), unknowns, masked))
    assert abs(lev.sum() - unknowns) <= R.sum() * tol
    # class and C-ABI, bit for bit
    ni = t.counts[2]
    ids = [ni - 1, 0, 3]
    c_cov, c_info, c_lev = h.pose_pose_leverages(hipapi.RES_IMU, ids)
    assert np.array_equal(c_cov, cov[sl][ids]) and np.array_equal(c_info, info[sl][ids])
    assert np.array_equal(c_lev, lev[sl][ids])
    a_cov, _, a_lev = h.pose_pose_leverages(hipapi.RES_IMU, None, count=ni)
    assert np.array_equal(a_cov, cov[sl]) and np.array_equal(a_lev, lev[sl])
    for i in ids:
        assert h.GetImuLeverage(i) == lev[sl][i]
    assert h.GetUnaryLeverage(1) == lev[t.kind_slice(hipapi.RES_UNARY)][1]
    assert h.GetBinaryLeverage(2) == lev[t.kind_slice(hipapi.RES_BINARY)][2]
    with pytest.raises(RuntimeError, match="unavailable"):
        h.GetImuLeverage(ni)
    with pytest.raises(RuntimeError, match="unavailable"):
        h.pose_pose_leverages(hipapi.RES_BINARY, [t.counts[1]])
    del eng, h
    gc.collect()


def test_pose_graph_application_prints_leverages():
    """applications/unary_binary_imu_test --leverages (LmSize 0, PoseSize 9, the committed log.dat): one line for the
    41 position fixes and one for the 40 inertial residuals, and the solution printed before them is the one the
    program prints without the flag."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ba_amd", "lib", "unary_binary_imu_test")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    log = os.path.join(root, "applications", "unary_binary_imu_test", "log.dat")
    plain = subprocess.run([exe, log], capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe, log, "--leverages"], capture_output=True, text=True, timeout=120)
    assert r.returncode == plain.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    lev = {ln.split()[1]: ln.split() for ln in lines if ln.startswith("LEVERAGES")}
    assert [ln for ln in lines if not ln.startswith("LEVERAGES")] == plain.stdout.splitlines()
    assert set(lev) == {"unary", "inertial"}
    for kind, count in (("unary", 41), ("inertial", 40)):
        w = lev[kind]
        assert w[2] == "count" and int(w[3]) == count and w[4] == "median" and w[6] == "max"
        med, top = float(w[5]), float(w[7])
        print("%s: median %.6g, largest %.6g" % (kind, med, top))
        assert np.isfinite(med) and np.isfinite(top) and 0.0 < med <= top


# ---- refusals and ownership --------------------------------------------------------------------------------
def test_refusals():
    """Each refusal carries a message that names the call, and the engine stays usable after it."""
    eng = _graph_engine(finalize=False)[0]
    with pytest.raises(hipapi.HipError, match=CALL + "ba_hip_finalize has not been called"):
        eng.pose_pose_leverages(hipapi.RES_UNARY, [0])
    eng.close()
    sc = scene.make_scene(12, 60, 4, lm_dim=1, seed=11)
    s = lc.engine(sc, 1, _fixed(sc), pose_pose=True)
    eng = s.eng
    nu, nb, _ = pc.helper_terms(sc, sc.num_poses).counts
    with pytest.raises(hipapi.HipError, match=CALL + "needs the factor"):
        eng.pose_pose_leverages(hipapi.RES_UNARY)
    lc.solve(s)
    want = eng.pose_pose_leverages(hipapi.RES_BINARY)
    assert want[0].shape == (nb, 15, 15)
    with pytest.raises(hipapi.HipError, match=CALL + "kind 3 is none of"):
        eng.pose_pose_leverages(3, [0])
    with pytest.raises(hipapi.HipError, match=CALL + "id %d is not a binary residual" % nb):
        eng.pose_pose_leverages(hipapi.RES_BINARY, [0, nb])
    with pytest.raises(hipapi.HipError, match=CALL + "id 0 is not an inertial residual"):
        eng.pose_pose_leverages(hipapi.RES_IMU, [0])
    with pytest.raises(hipapi.HipError, match=CALL + "with NULL ids n must be the residual count"):
        eng.pose_pose_leverages(hipapi.RES_UNARY, None, count=nu - 1)
    with pytest.raises(hipapi.HipError, match=CALL + "every output is NULL"):
        eng.pose_pose_leverages(hipapi.RES_UNARY, [0], want=(False, False, False))
    assert eng.pose_pose_leverages(hipapi.RES_IMU)[2].shape == (0,)
    assert np.array_equal(eng.pose_pose_leverages(hipapi.RES_BINARY, [1])[0], want[0][[1]])
    eng.linearize()
    with pytest.raises(hipapi.HipError, match=CALL + ".*re-linearised"):
        eng.pose_pose_leverages(hipapi.RES_BINARY, [1])
    eng.set_reduced_solver(hipapi.SOLVER_PCG)
    lc.solve(s)
    with pytest.raises(hipapi.HipError, match=CALL + ".*PCG"):
        eng.pose_pose_leverages(hipapi.RES_BINARY, [1])
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    lc.solve(s)
    got = eng.pose_pose_leverages(hipapi.RES_BINARY)
    # (the unary Huber scales compound over the linearisations: the system has moved, the call is served again)
    assert got[0].shape == want[0].shape and np.all(np.isfinite(got[0]))
    eng.release_marginals()
    assert np.array_equal(eng.pose_pose_leverages(hipapi.RES_BINARY, [2, 0])[2], got[2][[2, 0]])
    eng.close()


def test_ownership():
    """Nothing is allocated before the first request, a request keeps nothing beyond the Sigma store, and after
    ba_hip_release_marginals and close() the byte count of the process is back where it started."""
    live = hipapi.device_bytes_live
    base = live()
    eng, sc, t, pa, masks = _graph_engine()
    after_solve = live()
    assert after_solve > base
    eng.pose_pose_leverages(hipapi.RES_BINARY)
    with_store = live()
    assert with_store > after_solve
    eng.pose_pose_leverages(hipapi.RES_UNARY)
    eng.pose_pose_leverages(hipapi.RES_BINARY, [3, 1])
    assert live() == with_store
    eng.release_marginals()
    assert live() == after_solve
    eng.close()
    assert live() == base
