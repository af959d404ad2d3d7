"""Levenberg-Marquardt damping on the device (ba_hip_set_damping) against numpy.

The reference is numpy only (damping_cases.engine_system): the dense H and g of a small scene from the engine's own
whitened Jacobians of an UNDAMPED linearisation, its unreduced right-hand sides, and the pose-pose blocks from the S of
the same scene with every landmark inactive (nothing eliminated); masks applied; damped and solved densely.  The scenes
sit at the kernels' edges (damping_cases.edge_problem: n = 66, tracks of 1, 2, 63, 64, 65, 129 and 0 observations,
masks 0x7 and 0x38, unary priors, binary edges with a duplicate and a reversed pair; inertial_problem: PoseSize 15).

Bounds, those of the parity tests for the same quantities (test_pose_graph_unary_binary / test_visual_inertial): 1e-11
on S and on the damping diagonal per entry, 1e-10 on the gradient — both per block, relative to the block's scale
(posepose_cases.block_errors) — 1e-9 on delta and on the predicted decrease.  Every test prints the figures it asserts
("DAMPING ..." lines, pytest -s).

The rejected Gauss-Newton start was found on the CPU with the oracle: OracleBundleAdjuster(3, 6) on
scene.make_scene(14, 60, 4, lm_dim=3, seed=1, trans_sigma=0.3, rot_sigma=0.05, depth_sigma=0.3, outlier_frac=0) with
the two anchors fixed and gn_options ends Solve(10) in ErrorIncreased at its first step, with the robust norm and
without it (seeds 1, 2, 3 and 5 all do)."""
import ctypes

import numpy as np
import pytest

import damping_cases as dc
import leverage_cases as lc
import posepose_cases as pp
from ba_amd import adjuster, hipapi, scene
from helpers import fill, rel_err

pytestmark = pytest.mark.gpu

LAMBDAS = (1e-4, 1.0, 1e4)
TOL_S, TOL_G, TOL_DELTA = 1e-11, 1e-10, 1e-9
DAMPED = "the linearisation the device holds is damped \\(ba_hip_set_damping\\), linearise and solve once with damping 0"
u32p, u8p, dp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)


def _report(tag, **figs):
    print("DAMPING %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in figs.items())), flush=True)


def _p(a, t):
    return a.ctypes.data_as(t)


def _engine(pr, pivot_tol=0.0, keys=None, landmarks_active=True):
    """the whole problem in an engine (Huber weights on, the reduced system kept), finalized, masks set"""
    sc = pr.sc
    eng = hipapi.Engine(pr.LM, pr.D)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.keep_reduced_system = 1
    o.gyro_sigma, o.accel_sigma = 5.3088444e-5, 0.001883649
    o.gyro_bias_sigma, o.accel_bias_sigma = 1.4125375e-4, 1.2589254e-2
    o.pivot_rel_tolerance = pivot_tol
    eng.set_options(o)
    for k, v in (keys or {}).items():
        eng.debug_set(k, v)
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, v_w=pr.vel, b=pr.bias, is_active=pr.pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose, is_active=pr.la if landmarks_active else np.zeros_like(pr.la))
    eng.set_projection_residuals(pr.z, pr.opose, pr.olm)
    if len(pr.un):
        rot = np.ones(len(pr.un), np.uint8)
        eng._chk(eng.L.ba_hip_set_unary_residuals(eng.h, len(pr.un), _p(pr.un, u32p), _p(pr.un_t, dp), _p(pr.un_ci, dp), _p(rot, u8p)))
    if len(pr.b1):
        w, rot = np.ones(len(pr.b1)), np.ones(len(pr.b1), np.uint8)
        eng._chk(eng.L.ba_hip_set_binary_residuals(eng.h, len(pr.b1), _p(pr.b1, u32p), _p(pr.b2, u32p), _p(pr.b_t, dp), _p(pr.b_ci, dp),
                                                   _p(pr.b_cs, dp), _p(w, dp), _p(rot, u8p)))
    if len(pr.i1):
        meas = [sc.imu_meas[i] for i in pr.i1]
        assert min(len(m) for m in meas) >= 3
        ptr = np.zeros(len(meas) + 1, np.uint32)
        ptr[1:] = np.cumsum([len(m) for m in meas])
        m7 = np.ascontiguousarray(np.concatenate(meas))
        w = np.ones(len(meas))
        eng._chk(eng.L.ba_hip_set_gravity(eng.h, _p(np.ascontiguousarray(sc.gravity, dtype=np.float64), dp)))
        eng._chk(eng.L.ba_hip_set_imu_residuals(eng.h, len(meas), _p(pr.i1, u32p), _p(pr.i2, u32p), _p(ptr, u32p), _p(m7, dp), _p(w, dp)))
    eng.set_pose_ordering(hipapi.ORDER_NATURAL)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(pr.masks)
    return eng


def _setup(pr, eng):
    s = lc.Setup()
    s.eng, s.sc, s.pa, s.la, s.lm_dim, s.D, s.K = eng, pr.sc, pr.pa, pr.la, pr.LM, pr.D, 0
    s.obs_pose, s.obs_lm = pr.opose.astype(np.int64), pr.olm.astype(np.int64)
    s.masks = pr.masks
    return s


def _state(eng, nres):
    """what one linearisation and solve leave: everything the bitwise comparisons look at"""
    a, b, c = eng.get_rhs()
    return dict(S=eng.get_S(), rhs_sc=a, rhs_p=b, rhs_l=c, delta=np.concatenate(eng.get_delta_gn()),
                rows=np.concatenate([x.ravel() for x in eng.get_proj_jacobians(nres)]), w=eng.get_proj_weights(nres))


PROBLEMS = {"edge_lm1": lambda: dc.edge_problem(1), "edge_lm3": lambda: dc.edge_problem(3), "inertial": dc.inertial_problem}
_refs = {}


def _reference(name):
    """(problem, undamped state, H, g, n, masked) of a scene: computed once, shared, read-only"""
    if name not in _refs:
        pr = PROBLEMS[name]()
        bare = _engine(pr, landmarks_active=False)     # no landmark is eliminated: its S is the pose block U of H
        bare.linearize()
        U_engine = bare.get_S()
        bare.close()
        eng = _engine(pr)
        eng.linearize()
        assert eng.solve_gn() == 0
        st = _state(eng, len(pr.opose))
        assert eng.damping_terms()["lambda"] == 0.0
        H, g, n, masked = dc.engine_system(_setup(pr, eng), U_engine, st["rhs_p"], st["rhs_l"], dc.pose_pose_pairs(pr))
        eng.close()
        for v in list(st.values()) + [H, g, masked]:
            v.setflags(write=False)
        _refs[name] = (pr, st, H, g, n, masked)
    return _refs[name]


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_damped_step_matches_the_dense_reference(name, lam):
    pr, st0, H, g, n, masked = _reference(name)
    D, LM = pr.D, pr.LM
    delta_ref, d_ref, pred_ref = dc.dense_step(H, g, lam, masked)
    Hl = H + lam * np.diag(d_ref)
    U, W, V = Hl[:n, :n], Hl[:n, n:], Hl[n:, n:]
    Vi = np.linalg.inv(V)
    S_ref, rhs_ref = U - W @ Vi @ W.T, g[:n] - W @ Vi @ g[n:]
    # the scale of a block: the magnitudes of its terms (the fixed 1e6 of a masked parameter is not one of them)
    M = np.abs(U) + np.abs(W) @ np.abs(Vi) @ np.abs(W).T
    M[masked, masked] = 0.0
    nb = n // D
    scale = M.reshape(nb, D, nb, D).max(axis=(1, 3))
    g_scale = (np.abs(g[:n]) + np.abs(W) @ np.abs(Vi) @ np.abs(g[n:])).reshape(nb, D).max(axis=1)

    eng = _engine(pr)
    eng.set_damping(lam)
    eng.linearize()
    assert eng.solve_gn() == 0
    d_p, d_l = eng.damping_diagonal()
    S, (rhs_sc, rhs_p, rhs_l) = eng.get_S(), eng.get_rhs()
    delta = np.concatenate(eng.get_delta_gn())
    terms = eng.damping_terms()
    res, rel = eng.check_solve()           # get_S and check_solve serve the damped S
    eng.close()

    seen = np.repeat(np.bincount(pr.olm, minlength=len(pr.la))[pr.la.astype(bool)] > 0, LM)
    assert np.array_equal(d_l[~seen], np.zeros(int((~seen).sum())))   # a landmark without observations is never linearised
    free = np.ones(n, dtype=bool)
    free[masked] = False
    assert np.array_equal(d_p[masked], np.zeros(len(masked)))
    e_S = pp.block_errors(S, S_ref, scale, D)
    figs = dict(
        lam=lam, cond=np.linalg.cond(Hl), d_p=np.abs(d_p[free] / d_ref[:n][free] - 1).max(),
        d_l=np.abs(d_l[seen] / d_ref[n:][seen] - 1).max(), S=e_S.worst,
        rhs=pp.vector_block_error(rhs_sc, rhs_ref, g_scale, D), delta=rel_err(delta, delta_ref),
        pred=abs(terms["predicted_decrease"] - pred_ref) / pred_ref,
        dDd=abs(terms["step_scaled_sq"] - delta_ref @ (d_ref * delta_ref)) / (delta_ref @ (d_ref * delta_ref)),
        check_solve=res / rel)
    _report("%s" % name, **figs)
    assert terms["lambda"] == lam and terms["device_ms"] > 0
    dd = np.concatenate([d_p[free], d_l[seen]])
    assert terms["diag_min"] == dd.min() and terms["diag_max"] == dd.max()
    assert np.array_equal(rhs_p, st0["rhs_p"]) and np.array_equal(rhs_l, st0["rhs_l"])   # g itself is not damped
    assert figs["d_p"] <= TOL_S and figs["d_l"] <= TOL_S
    assert pp.accepted(e_S, TOL_S), (e_S.worst, e_S.where, e_S.spurious, e_S.missing)
    assert figs["rhs"] <= TOL_G
    assert figs["delta"] <= TOL_DELTA
    assert figs["pred"] <= TOL_DELTA and figs["dDd"] <= TOL_DELTA
    assert pred_ref > 0 and figs["check_solve"] < 1e-9


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_damping_zero_is_the_undamped_engine(name):
    """after ba_hip_set_damping(0) — before any damping, and again after a damped linearisation — S, the right-hand
    sides, delta, the Jacobian rows, the weights and the errors are bitwise those of an engine that never saw the call
    and linearised as often (every linearisation compounds the Huber scales of the unary residuals), and until a
    damping is set no damping buffer exists"""
    pr = _reference(name)[0]
    nres = len(pr.opose)

    def round_(eng):
        errs = eng.linearize()
        assert eng.solve_gn() == 0
        st = _state(eng, nres)
        st["errors"] = np.array([errs.proj_error, errs.unary_error, errs.binary_error, errs.inertial_error])
        return st
    base = hipapi.device_bytes_live()
    clean = _engine(pr)
    want = [round_(clean) for _ in range(3)]
    bytes_clean = hipapi.device_bytes_live() - base
    clean.close()
    assert hipapi.device_bytes_live() == base

    eng = _engine(pr)
    eng.set_profiling(1)
    eng.set_damping(0.0)
    first = round_(eng)
    k0 = eng.kernel_stats()
    with pytest.raises(hipapi.HipError, match="is not damped"):
        eng.damping_diagonal()
    eng.set_damping(1.0)
    damped = round_(eng)
    bytes_damped = hipapi.device_bytes_live() - base
    eng.set_damping(0.0)
    again = round_(eng)
    k1 = eng.kernel_stats()
    eng.close()
    for k in want[0]:
        assert np.array_equal(first[k], want[0][k]), k
        assert np.array_equal(again[k], want[2][k]), k
    assert not np.array_equal(damped["S"], want[1]["S"]) and not np.array_equal(damped["delta"], want[1]["delta"])
    assert np.array_equal(damped["w"], want[1]["w"]) and np.array_equal(damped["rhs_p"], want[1]["rhs_p"])
    # the profiled launches of a linearisation are the same with and without damping: the damped linearisation is an
    # instantiation of the same launch, the damping kernels are not among the profiled ones
    assert k1.landmarks_launches == 3 * k0.landmarks_launches and k1.pose_blocks_launches == 3 * k0.pose_blocks_launches
    # d_p (ld doubles), d_l, the Schur diagonals, the partials and the four sums: what a damped linearisation allocates
    assert bytes_damped > bytes_clean
    _report("%s bytes" % name, undamped=bytes_clean, damped=bytes_damped)

    # with the damping at 0 throughout, the engine holds what an engine that never saw the call holds
    eng = _engine(pr)
    eng.set_damping(0.0)
    for _ in range(3):
        round_(eng)
    assert hipapi.device_bytes_live() - base == bytes_clean, "ba_hip_set_damping(0) allocated something"
    eng.close()


def test_pcg_and_direct_solve_agree_under_damping():
    pr, _, H, g, n, masked = _reference("edge_lm1")
    tol = 1e-10
    delta_ref, d_ref, _ = dc.dense_step(H, g, 1.0, masked)
    Hl = H + np.diag(d_ref)
    cond = np.linalg.cond(Hl[:n, :n] - Hl[:n, n:] @ np.linalg.solve(Hl[n:, n:], Hl[n:, :n]))
    out = []
    for mode in (hipapi.SOLVER_DIRECT, hipapi.SOLVER_PCG):
        eng = _engine(pr)
        eng.set_reduced_solver(mode, rel_tolerance=tol)
        eng.set_damping(1.0)
        eng.linearize()
        assert eng.solve_gn() == 0
        out.append(np.concatenate(eng.get_delta_gn()))
        if mode == hipapi.SOLVER_PCG:
            assert eng.pcg_stats()["converged"]
            with pytest.raises(hipapi.HipError, match=DAMPED):
                eng.pcg_panel_solve_system(np.eye(n)[:, :2], rel_tolerance=1e-8)
        eng.close()
    err = rel_err(out[1], out[0])
    _report("pcg against direct", err=err, bound=cond * tol, cond=cond, against_numpy=rel_err(out[1], delta_ref))
    assert err <= cond * tol + 4.5 * dc.EPS * cond


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_kernel_variants_stay_bitwise_identical_under_damping(lm_dim):
    """every ba_hip_debug_set variant that test_track_lengths_gpu.py holds bitwise equal without damping gives
    bitwise the same damped system, right-hand sides, weights, rows and damping diagonal with lambda = 1"""
    pr = _reference("edge_lm%d" % lm_dim)[0]
    nres = len(pr.opose)

    def run(keys):
        eng = _engine(pr, keys=keys)
        eng.set_damping(1.0)
        eng.linearize()
        assert eng.solve_gn() == 0
        st = _state(eng, nres)
        st["d_p"], st["d_l"] = eng.damping_diagonal()
        eng.close()
        return st
    base = run({})
    assert np.isfinite(base["S"]).all() and np.abs(base["S"]).max() > 0
    for keys in ({4: 1}, {1: 0}, {1: 1}, {1: 2}, {1: 6}, {2: 1}, {3: 1}, {5: 1}):
        st = run(keys)
        for k, v in base.items():
            assert np.array_equal(st[k], v), (keys, k)


def test_singular_scene_is_solved_with_damping():
    """all-active monocular scene, only the root masked: the scale about the root is free, the undamped S is singular
    and the direct solve reports it; with lambda = 1e-4 the system is positive definite, the step has a positive gain
    ratio and lowers the error"""
    pr = dc.singular_problem()
    tol = 1e-8      # between the singular pivot (5e-12 of its diagonal entry on the CPU) and the next one (1e-2)
    eng = _engine(pr, pivot_tol=tol)
    eng.linearize()
    S = eng.get_S()
    ev = np.linalg.eigvalsh(S)
    _report("singular S", eig_min=ev[0], eig_next=ev[1], max_diag=np.diag(S).max())
    assert abs(ev[0]) < tol * np.diag(S).max() < ev[1]
    assert eng.solve_gn() == 4      # BA_HIP_FACTORIZATION_ERROR
    eng.set_damping(1e-4)
    eng.linearize()
    assert eng.solve_gn() == 0
    terms = eng.damping_terms()
    eng.compose_step(0.0, 1.0)
    pre = eng.eval_residuals().total()
    eng.apply_step()
    post = eng.eval_residuals().total()
    rho = (pre - post) / terms["predicted_decrease"]
    _report("singular damped", pre=pre, post=post, pred=terms["predicted_decrease"], rho=rho)
    assert rho > 0 and post < pre
    eng.close()


def _lm_scene():
    sc = scene.make_scene(14, 60, 4, lm_dim=3, seed=1, trans_sigma=0.3, rot_sigma=0.05, depth_sigma=0.3, outlier_frac=0.0)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    return sc, pa


def _adjuster(sc, pa, lm):
    h = adjuster.BundleAdjuster(3, 6)
    opt = adjuster.default_options()
    opt.use_dogleg = 0
    opt.use_robust_norm_for_proj_residuals = 0     # fixed weights: the errors of successive iterations compare
    opt.error_change_threshold = 0
    opt.param_change_threshold = 0
    h.Init(opt)
    if lm:
        h.SetLevenbergMarquardt(True, 1e-4)
    fill(h, sc, active=pa)
    return h


def test_levenberg_marquardt_recovers_a_start_that_gauss_newton_rejects():
    sc, pa = _lm_scene()
    gn = _adjuster(sc, pa, False)
    gn.Solve(10)
    assert adjuster.RESULT_NAMES[gn.summary().result] == "ErrorIncreased"
    h = _adjuster(sc, pa, True)
    assert h.damping() == 1e-4
    start, accepted, rejected, shrank = None, [], 0, 0
    for it in range(10):
        before = h.damping()
        h.Solve(1)
        s = h.summary()
        rho, rej = h.levenberg_marquardt_state()
        _report("lm iteration %d" % it, lam_before=before, lam_after=h.damping(), rho=rho, rejected=rej, pre=s.pre_solve_norm,
                post=s.post_solve_norm, result=s.result)
        assert adjuster.RESULT_NAMES[s.result] == "Success"
        start = s.pre_solve_norm if start is None else start
        assert rho > 0 and s.post_solve_norm < s.pre_solve_norm        # an accepted step never raises the error
        if accepted:
            assert s.pre_solve_norm <= accepted[-1] * (1 + 1e-9)
        accepted.append(s.post_solve_norm)
        rejected += rej
        shrank += rej == 0 and h.damping() < before
    assert rejected >= 1, "no inner rejection: the re-linearise path did not run"
    assert shrank >= 1
    assert accepted[-1] < start


def test_readers_refuse_a_damped_factor_and_serve_again():
    pr = _reference("edge_lm1")[0]
    n = 6 * int(pr.pa.sum())
    B = np.random.default_rng(3).normal(size=(n, 2))
    # marginalise the free, unmasked pose that anchors the most landmarks, with the landmarks anchored in it
    anchored = np.bincount(pr.sc.lm_ref_pose[np.unique(pr.olm)], minlength=pr.P) * (pr.pa > 0) * (pr.masks == 0)
    m_pose = int(np.argmax(anchored))
    m_lms = np.nonzero(pr.sc.lm_ref_pose == m_pose)[0]
    assert anchored[m_pose] >= 3
    readers = {
        "ba_hip_compute_marginals": lambda e: e.compute_marginals(),
        "ba_hip_get_joint_marginals": lambda e: e.joint_marginals([2, 9]),
        "ba_hip_get_projection_leverages": lambda e: e.projection_leverages([0, 5]),
        "ba_hip_factor_solve": lambda e: e.factor_solve(B),
        "ba_hip_get_weakest_modes": lambda e: e.weakest_modes(2),
        "marginalize": lambda e: e.marginalize([m_pose], m_lms),
    }
    clean = _engine(pr)
    for _ in range(2):      # (as often as the engine below: every linearisation compounds the unary Huber scales)
        clean.linearize()
        assert clean.solve_gn() == 0
    want = clean.pose_marginals([2, 9])
    clean.close()

    eng = _engine(pr)
    eng.set_damping(1.0)
    eng.linearize()
    assert eng.solve_gn() == 0
    for who, call in readers.items():
        with pytest.raises(hipapi.HipError, match=who + ": " + DAMPED):
            call(eng)
    with pytest.raises(hipapi.HipError, match="ba_hip_dogleg_terms: the linearisation the device holds is damped"):
        eng.dogleg_terms(1)
    eng.get_S()
    eng.check_solve()
    eng.set_damping(0.0)
    for who, call in readers.items():          # setting the damping back does not make the held factor undamped
        with pytest.raises(hipapi.HipError, match=who + ": " + DAMPED):
            call(eng)
    eng.linearize()
    assert eng.solve_gn() == 0
    got = eng.pose_marginals([2, 9])
    assert np.array_equal(np.asarray(got), np.asarray(want))
    for who, call in readers.items():
        call(eng)
    eng.dogleg_terms(1)
    eng.close()


def test_damping_is_refused_with_calibration_and_on_hooked_engines():
    eng = hipapi.Engine(1, 6)
    eng.set_calibration(0, True)
    with pytest.raises(hipapi.HipError, match="ba_hip_set_damping: not offered with calibration unknowns"):
        eng.set_damping(1.0)
    eng.set_damping(0.0)
    eng.close()
    eng = hipapi.Engine(1, 6)
    eng.set_damping(1.0)
    with pytest.raises(hipapi.HipError, match="damping is set"):
        eng.set_calibration(0, True)
    eng.close()
    eng = hipapi.Engine(1, 6)
    eng.set_allreduce(lambda ptr, count, dtype: 0, 0, 1)
    with pytest.raises(hipapi.HipError, match="ba_hip_set_damping: not offered on sharded engines or with the distributed solve"):
        eng.set_damping(1.0)
    with pytest.raises(hipapi.HipError, match="lambda must be finite"):
        eng.set_damping(-1.0)
    eng.close()
