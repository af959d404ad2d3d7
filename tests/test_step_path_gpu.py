"""The step path on the MI355X -- what runs between the reduced solve and the next linearisation -- against the
long-double reference of step_cases.py, read through the existing taps only: get_rhs, get_delta_gn, get_step,
get_proj_jacobians, get_calib_jacobians, get_poses, get_landmarks, get_landmark_flags, get_cameras, dogleg_terms,
compose_step, apply_step, rollback, eval_residuals, end_solve.  One engine per case, everything read once (_run);
test_step_path.py shows on the CPU that the bounds hold for the oracle and a float64 restatement and that the
comparator rejects thirteen wrong step paths.  Every test prints its worst figure and where it occurred (pytest -s).

The rungs of the update ladder are not applied to `tvs`: after a rejected step the reference keeps the rejected
camera mount in the rig (BundleAdjuster.cpp:1060-1068, mirrored by ba_hip_rollback), so a rollback does not restore
the state there by design; that case composes its steps, applies one and ends the solve."""
import ctypes
import threading
import types

import numpy as np
import pytest

import step_cases as sc
from ba_amd import hipapi, sharding

pytestmark = pytest.mark.gpu

dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
CASES = sorted(sc.CASES)
REAL_STEP = 0.5                     # the step applied for good: half the Gauss-Newton step


def _engine(c, ids=None, oracle_options=None):
    """the case (or the landmarks `ids` of it with their residuals) in an engine, linearisation pending"""
    sce = c.sc
    ids = np.arange(c.L) if ids is None else np.asarray(ids)
    new_id = np.full(c.L, -1, dtype=np.int64)
    new_id[ids] = np.arange(len(ids))
    sel = new_id[c.lm] >= 0
    eng = hipapi.Engine(c.LM, c.D)
    o = hipapi.Options()
    o.projection_outlier_threshold, o.use_robust_norm_for_proj_residuals = 1.0, 1
    o.use_triangular_matrices, o.keep_reduced_system = 1, 1
    if oracle_options is not None:
        for k in ("gyro_sigma", "accel_sigma", "gyro_bias_sigma", "accel_bias_sigma", "use_robust_norm_for_inertial_residuals"):
            setattr(o, k, getattr(oracle_options, k))
    eng.set_options(o)
    if c.K:
        eng.set_calibration(0, do_tvs=True)
    eng.set_cameras(sce.cam_params, c.t_vs)
    if c.imu:
        eng._chk(eng.L.ba_hip_set_gravity(eng.h, np.ascontiguousarray(sce.gravity, dtype=np.float64).ctypes.data_as(dp)))
    eng.set_poses(sce.poses, v_w=getattr(sce, "init_vel", None), b=getattr(sce, "init_bias", None), is_active=c.pa)
    eng.set_landmarks(sce.landmarks[ids], sce.lm_ref_pose[ids], is_active=c.la[ids])
    eng.set_projection_residuals(c.z[sel], c.pose[sel], new_id[c.lm[sel]].astype(np.uint32))
    if c.imu:
        ni = c.P - 1
        ptr = np.zeros(ni + 1, np.uint32)
        ptr[1:] = np.cumsum([len(m) for m in sce.imu_meas])
        m7 = np.ascontiguousarray(np.concatenate([np.asarray(m).reshape(-1, 7) for m in sce.imu_meas]))
        p1 = np.arange(ni, dtype=np.uint32)
        p2, w = p1 + 1, np.ones(ni)
        eng._chk(eng.L.ba_hip_set_imu_residuals(eng.h, ni, p1.ctypes.data_as(u32p), p2.ctypes.data_as(u32p),
                                                ptr.ctypes.data_as(u32p), m7.ctypes.data_as(dp), w.ctypes.data_as(dp)))
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(c.masks)
    return eng, np.nonzero(sel)[0]


def _scalars(s):
    return {k: getattr(s, k) for k in sc.SCALARS}


def _lin(eng, c, n_obs):
    jm, jr, jl, r = eng.get_proj_jacobians(n_obs)
    return types.SimpleNamespace(jm=jm, jr=jr, jl=jl, r=r, jk=eng.get_calib_jacobians(n_obs) if c.K else None)


def _state(eng, c, rho=None):
    poses, vel, bias = eng.get_poses(c.P)
    rel, _ = eng.get_landmark_flags(c.L)
    return types.SimpleNamespace(poses=poses, vel=vel, bias=bias, lms=eng.get_landmarks(c.L) if c.LM == 3 else None,
                                 rho=rho, rel=rel)


def _same_state(a, b, c):
    return (np.array_equal(a.poses, b.poses) and np.array_equal(a.vel, b.vel) and np.array_equal(a.bias, b.bias)
            and np.array_equal(a.rel, b.rel) and (c.LM != 3 or np.array_equal(a.lms, b.lms)))


def _errors(e):
    return (e.proj_error, e.binary_error, e.unary_error, e.inertial_error)


def _step(eng, a, b):
    nrm = eng.compose_step(a, b)
    step_p, step_l = eng.get_step()
    return types.SimpleNamespace(a=a, b=b, step_p=step_p, step_l=step_l, norm_p=nrm.step_p_norm, norm_l=nrm.step_l_norm)


_runs = {}


def _run(po, name):
    if name in _runs:
        return _runs[name]
    c = sc.case(name)
    oo = po.default_options() if c.imu else None
    r = types.SimpleNamespace(case=c)
    # a fresh engine whose ONLY dogleg call comes after the solve; ended without a step, it also shows the inverse
    # depths the device starts from (k_sensor_to_world copies them into x_w[3])
    fresh, _ = _engine(c, oracle_options=oo)
    fresh.linearize()
    assert fresh.solve_gn() == 0
    r.scal_fresh = _scalars(fresh.dogleg_terms(1))
    fresh.end_solve()
    rho0 = np.ascontiguousarray(fresh.get_landmarks(c.L)[:, 3]) if c.LM == 1 else None
    fresh.close()
    # 1. linearise; the dogleg sums before the solve
    eng, _ = _engine(c, oracle_options=oo)
    r.built = eng.linearize()
    b = types.SimpleNamespace(case=c, lin=_lin(eng, c, c.O))
    _, b.rhs_p, b.rhs_l = eng.get_rhs()
    b.scal0 = _scalars(eng.dogleg_terms(0))
    # 2. solve; the sums again (the denominator reused)
    assert eng.solve_gn() == 0
    b.gn_p, b.gn_l = eng.get_delta_gn()
    b.scal1 = _scalars(eng.dogleg_terms(1))
    # 4. the ladder: compose, read, apply, read, roll back
    state0 = _state(eng, c, rho0)
    eval0 = _errors(eng.eval_residuals())
    b.steps, b.updates, r.rollbacks = [], [], []
    if not c.K:
        coefs = sc.ladder_coefficients(c, b.gn_p)
        if c.LM == 1:
            coefs.append(sc.negative_coefficient(c, rho0, b.gn_l))
        for k, coef in enumerate(coefs):
            s = _step(eng, 0.0, coef)
            eng.apply_step()
            after = _state(eng, c)
            eng.rollback()
            back = _state(eng, c, rho0)
            r.rollbacks.append(_same_state(back, state0, c) and _errors(eng.eval_residuals()) == eval0)
            b.steps.append(s)
            b.updates.append(types.SimpleNamespace(step_p=s.step_p, step_l=s.step_l, before=state0, after=after))
    # 5. mixed steps
    b.steps += [_step(eng, 0.3, 0.5), _step(eng, 0.7, 0.0)]
    # 6. one moderate step for good, the next linearisation
    s = _step(eng, 0.0, REAL_STEP)
    eng.apply_step()
    state1 = _state(eng, c)
    b.steps.append(s)
    b.updates.append(types.SimpleNamespace(step_p=s.step_p, step_l=s.step_l, before=state0, after=state1))
    r.built2 = eng.linearize()
    b2 = types.SimpleNamespace(case=c, lin=_lin(eng, c, c.O), system=False, gn_p=b.gn_p, gn_l=b.gn_l)
    _, b2.rhs_p, b2.rhs_l = eng.get_rhs()
    b2.scal0 = _scalars(eng.dogleg_terms(0))
    b2.steps = [_step(eng, 0.7, 0.0)]            # the Gauss-Newton buffers still hold the previous solve
    r.gn_kept = all(np.array_equal(x, y) for x, y in zip(eng.get_delta_gn(), (b.gn_p, b.gn_l)))
    # 7. end of the solve
    eng.end_solve()
    if c.LM == 1:
        t_vs1 = eng.get_cameras(1)[0] if c.K else c.t_vs
        rho1 = sc.update_reference(c, state0, s.step_p, s.step_l).rho
        b.world = types.SimpleNamespace(x_w0=c.sc.landmarks, poses0=c.sc.poses, t_vs0=c.t_vs, poses1=state1.poses,
                                        t_vs1=t_vs1, rho1=rho1, x_w1=eng.get_landmarks(c.L), rho0=rho0)
        r.t_vs1, r.tail = t_vs1, s.step_p[c.n:]
    eng.close()
    r.b, r.b2 = b, b2
    _runs[name] = r
    return r


_oracles = {}


def _oracle(po, name):
    if name not in _oracles:
        c = sc.case(name)
        o = sc.oracle_run(po, c)
        (lm, _), (pose, _) = sc.system_ratios(c, o.lin, o.gn_p, o.gn_l)
        _oracles[name] = (o, (lm, pose))
    return _oracles[name]


def _pose_pose_part(po, c, o, rhs_p):
    """(the inertial residuals' part of j_rhs_sq from the oracle's Jacobians and informations, what it is known to):
    posepose_cases.j_rhs_sq, held to the 1e-9 of test_pose_pose_blocks_gpu.py::test_dogleg_denominator"""
    if not c.imu:
        return 0.0, 0.0
    import posepose_cases as pp
    t = pp.Terms()
    t.imu_p1 = np.arange(c.P - 1, dtype=np.uint32)
    t.imu_p2 = t.imu_p1 + 1
    dz, ci = pp.oracle_jacobians(o.ba, t)
    val = pp.j_rhs_sq(t, c.D, dz, ci, rhs_p[:c.n], c.pa, c.masks)
    return val, 1e-9 * val


@pytest.mark.parametrize("name", CASES)
def test_dogleg_sums_and_the_reused_denominator(oracle_lib, name):
    r = _run(oracle_lib, name)
    b, c = r.b, r.case
    for k in ("gn_p_sq", "gn_l_sq", "gn_k_sq", "rhs_gn_p", "rhs_gn_l", "rhs_gn_k"):
        assert b.scal0[k] == 0.0, k
    assert b.scal1["j_rhs_sq"] == b.scal0["j_rhs_sq"], "the reused denominator is not the one summed before the solve"
    assert b.scal1 == r.scal_fresh, "a first call after the solve does not return what the reusing call returns"
    o, _ = _oracle(oracle_lib, name)
    pp_jrhs, pp_tol = _pose_pose_part(oracle_lib, c, o, b.rhs_p)
    figs = sc.compare(types.SimpleNamespace(case=c, lin=b.lin, rhs_p=b.rhs_p, rhs_l=b.rhs_l, gn_p=b.gn_p, gn_l=b.gn_l,
                                            system=False, scal0=b.scal0, scal1=b.scal1, pp_jrhs=pp_jrhs, pp_tol=pp_tol))
    sc.report(name + " dogleg", figs)
    assert not sc.failures(figs), sc.failures(figs)
    assert len(figs) == 21
    if c.imu:
        # the inertial part dwarfs the projection part here; what it is known to (1e-9 of it) still leaves the projection
        # part, whose D-strided reads this case is for, resolved to three digits and more
        proj, scale = sc.dogleg_reference(c, b.lin, b.rhs_p, b.rhs_l, b.gn_p, b.gn_l, 0)["j_rhs_sq"]
        print("STEP %s: j_rhs_sq %.17g = projection part %.17g + inertial part %.17g (numpy on the oracle's Jacobians), "
              "tolerances %.3g and %.3g" % (name, b.scal1["j_rhs_sq"], float(proj), pp_jrhs,
                                            sc.chain_counts(c)["j_rhs_sq"] * sc.EPS * float(scale), pp_tol), flush=True)
        assert pp_tol < 1e-3 * float(proj)


@pytest.mark.parametrize("name", CASES)
def test_back_substitution_in_the_full_system(oracle_lib, name):
    r = _run(oracle_lib, name)
    b, c = r.b, r.case
    o, ratio = _oracle(oracle_lib, name)
    figs = sc.compare(types.SimpleNamespace(case=c, lin=b.lin, gn_p=b.gn_p, gn_l=b.gn_l), ratio)
    dl = np.linalg.norm(b.gn_l - o.gn_l) / np.linalg.norm(o.gn_l)
    print("STEP %s: full-system residual in eps, landmark rows: oracle %.3g, engine %.3g at row %s; pose rows: oracle %.3g, "
          "engine %s; delta_l against the oracle %.3g"
          % (name, ratio[0], figs["system.landmark_rows"].value, figs["system.landmark_rows"].where, ratio[1],
             "%.3g at row %s" % (figs["system.pose_rows"].value, figs["system.pose_rows"].where) if "system.pose_rows" in figs
             else "-", dl), flush=True)
    assert not sc.failures(figs), {k: vars(figs[k]) for k in sc.failures(figs)}
    assert dl < 1e-8


@pytest.mark.parametrize("name", CASES)
def test_steps_updates_and_rollbacks(oracle_lib, name):
    r = _run(oracle_lib, name)
    b, c = r.b, r.case
    figs = sc.compare(types.SimpleNamespace(case=c, rhs_p=b.rhs_p, rhs_l=b.rhs_l, gn_p=b.gn_p, gn_l=b.gn_l, steps=b.steps,
                                            updates=b.updates))
    sc.report(name + " steps", figs)
    assert not sc.failures(figs), {k: vars(figs[k]) for k in sc.failures(figs)}
    assert all(r.rollbacks), "a rollback does not restore the state (or the residuals) bit for bit: rung %s" % r.rollbacks
    if not c.K:
        assert len(r.rollbacks) == len(sc.ROTATION_LADDER) + (c.LM == 1)
        th = [np.linalg.norm(u.step_p[:c.n].reshape(-1, c.D)[:, 3:6], axis=1).max() for u in b.updates]
        assert th[0] == 0.0 and np.allclose(th[1:6], sc.ROTATION_LADDER[1:], rtol=1e-12)
        assert not b.steps[0].step_p.any() and not b.steps[0].step_l.any()
    if c.LM == 1 and not c.K:
        w = sc.update_reference(c, b.updates[6].before, b.updates[6].step_p, b.updates[6].step_l)
        assert 0 < len(w.negative) < c.L // 2 and (b.updates[6].after.rel == 0).sum() == len(w.negative)


@pytest.mark.parametrize("name", CASES)
def test_next_linearisation_serves_no_stale_sums(oracle_lib, name):
    r = _run(oracle_lib, name)
    b, b2, c = r.b, r.b2, r.case
    assert b2.scal0["j_rhs_sq"] != b.scal0["j_rhs_sq"], "dogleg_terms(0) served the denominator of the previous linearisation"
    assert r.gn_kept and np.abs(b.gn_p).max() > 0
    figs = sc.compare(b2)
    if c.imu:    # the pose-pose part of the denominator at the NEW state is not available from the oracle run at the old one
        del figs["scal0.j_rhs_sq"]
    sc.report(name + " relinearised", figs)
    assert not sc.failures(figs), {k: vars(figs[k]) for k in sc.failures(figs)}
    assert figs["step0.p_bitwise"].bound == 0 and "step0.l_bitwise" in figs


@pytest.mark.parametrize("name", [n for n in CASES if n != "edges_lm3"])
def test_world_coordinates_after_end_solve(oracle_lib, name):
    r = _run(oracle_lib, name)
    c = r.case
    figs = {}
    sc.compare_world(figs, c, r.b.world)
    sc.report(name + " world", figs)
    assert not sc.failures(figs), {k: vars(figs[k]) for k in sc.failures(figs)}
    if c.K:     # the mount after the applied step: exp_decoupled(T_vs, -delta_k), translation bitwise
        assert np.array_equal(r.t_vs1[:3], c.t_vs[:3] - r.tail[:3])
        q = sc._unit(sc.quat_mul(np.asarray(c.t_vs[3:7], dtype=sc.LD), sc.so3_exp(-np.asarray(r.tail[3:6], dtype=sc.LD))))
        assert np.abs(np.asarray(r.t_vs1[3:7], dtype=sc.LD) - q).max() <= sc.ROTATION_BOUND * sc.EPS


def test_negative_inverse_depths_after_end_solve(oracle_lib):
    """the rung that turns inverse depths negative, applied for good: end_solve shows the values the ladder cannot
    read (x_w[3] is the inverse depth) -- bitwise (rho - d) + d where rho - d < 0, rho - d elsewhere"""
    po = oracle_lib
    r = _run(po, "edges_lm1")
    c, b = r.case, r.b
    rho0 = r.b.world.rho0
    eng, _ = _engine(c)
    eng.linearize()
    assert eng.solve_gn() == 0
    s = _step(eng, 0.0, sc.negative_coefficient(c, rho0, b.gn_l))
    assert np.array_equal(s.step_l, b.steps[6].step_l)
    before = _state(eng, c, rho0)
    eng.apply_step()
    after = _state(eng, c)
    eng.end_solve()
    x_w1 = eng.get_landmarks(c.L)
    eng.close()
    w = sc.update_reference(c, before, s.step_p, s.step_l)
    figs = {}
    sc.compare_world(figs, c, types.SimpleNamespace(x_w0=c.sc.landmarks, poses0=c.sc.poses, t_vs0=c.t_vs, poses1=after.poses,
                                                    t_vs1=c.t_vs, rho1=w.rho, x_w1=x_w1, rho0=rho0))
    sc.report("edges_lm1 negative depths", figs)
    assert not sc.failures(figs), {k: vars(figs[k]) for k in sc.failures(figs)}
    assert len(w.negative) > 20 and (x_w1[:, 3] >= 0).all() and np.array_equal(after.rel, w.rel)


# ---- two shards -----------------------------------------------------------------------------------------------
def _shard_steps(eng, c, n_obs, out, key):
    try:
        q = types.SimpleNamespace()
        eng.linearize()
        q.lin = _lin(eng, c, n_obs)
        _, q.rhs_p, q.rhs_l = eng.get_rhs()
        q.scal0 = _scalars(eng.dogleg_terms(0))
        q.rc = eng.solve_gn()
        q.gn_p, q.gn_l = eng.get_delta_gn()
        q.scal1 = _scalars(eng.dogleg_terms(1))
        q.steps = [_step(eng, 0.3, 0.5), _step(eng, 0.7, 0.0)]
        out[key] = q
    except Exception as exc:  # surfaced by the assertions below
        out[key] = exc


def test_two_shards(oracle_lib):
    """`edges_lm1` dealt to two engines (threads and the in-process all-reduce, as test_two_shards_equal_one): both
    ranks report the same sums and norms bit for bit, and they hold the bounds against the reference assembled from
    the union of the shards' taps.  The pose-part sums are not summed across the shards (a sum over two ranks would
    be twice the reference)."""
    c = sc.case("edges_lm1")
    per_lm = np.bincount(c.lm, minlength=c.L)
    shards = sharding.landmark_shards(np.maximum(per_lm, 1), 2)
    engs, sels = zip(*[_engine(c, np.arange(lo, hi)) for lo, hi in shards])
    ar = sharding.ThreadAllReduce(2)
    for k in range(2):
        engs[k].set_allreduce(ar.hook(k), k, 2)
    out = {}
    th = [threading.Thread(target=_shard_steps, args=(engs[k], c, len(sels[k]), out, k)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    for e_ in engs:
        e_.close()
    assert not ar.failed
    for k in range(2):
        assert not isinstance(out[k], Exception), out[k]
    q0, q1 = out[0], out[1]
    assert q0.rc == q1.rc == 0
    assert q0.scal0 == q1.scal0 and q0.scal1 == q1.scal1
    assert np.array_equal(q0.rhs_p, q1.rhs_p) and np.array_equal(q0.gn_p, q1.gn_p)
    for s0, s1 in zip(q0.steps, q1.steps):
        assert (s0.norm_p, s0.norm_l) == (s1.norm_p, s1.norm_l) and np.array_equal(s0.step_p, s1.step_p)
    # the union: residuals of shard 0, then of shard 1; the landmark vectors in shard order are in optimisation order
    u = types.SimpleNamespace(**vars(c))
    order = np.concatenate(sels)
    u.z, u.pose, u.lm, u.ref = c.z[order], c.pose[order], c.lm[order], c.ref[order]
    cat = lambda f: np.concatenate([f(q0), f(q1)])
    lin = types.SimpleNamespace(jm=cat(lambda q: q.lin.jm), jr=cat(lambda q: q.lin.jr), jl=cat(lambda q: q.lin.jl),
                                r=cat(lambda q: q.lin.r), jk=None)
    steps = [types.SimpleNamespace(a=a.a, b=a.b, step_p=a.step_p, step_l=np.concatenate([a.step_l, b_.step_l]), norm_p=a.norm_p,
                                   norm_l=a.norm_l) for a, b_ in zip(q0.steps, q1.steps)]
    b = types.SimpleNamespace(case=u, lin=lin, rhs_p=q0.rhs_p, rhs_l=cat(lambda q: q.rhs_l), gn_p=q0.gn_p,
                              gn_l=cat(lambda q: q.gn_l), scal0=q0.scal0, scal1=q0.scal1, steps=steps)
    _, ratio = _oracle(oracle_lib, "edges_lm1")
    figs = sc.compare(b, ratio, shards=2)
    sc.report("two_shards", figs)
    print("STEP two_shards: full-system residual in eps, landmark rows %.3g (oracle %.3g), pose rows %.3g (oracle %.3g)"
          % (figs["system.landmark_rows"].value, ratio[0], figs["system.pose_rows"].value, ratio[1]), flush=True)
    assert not sc.failures(figs), {k: vars(figs[k]) for k in sc.failures(figs)}
    # replicated, not summed across the shards: the single engine's bits (its rhs_p differs from the all-reduced one in
    # the last bit of some entries, which these three sums do not resolve on this case)
    single = _run(oracle_lib, "edges_lm1").b
    differ = int((q0.rhs_p != single.rhs_p).sum())
    print("STEP two_shards: %d of %d entries of rhs_p differ from the single engine's, by at most %.3g relative"
          % (differ, len(single.rhs_p), np.abs(q0.rhs_p / np.where(single.rhs_p != 0, single.rhs_p, 1) - 1)[single.rhs_p != 0].max()),
          flush=True)
    for k in ("rhs_p_sq", "gn_p_sq", "rhs_gn_p"):
        assert q0.scal1[k] == single.scal1[k], k
    assert q0.scal0["rhs_p_sq"] == single.scal0["rhs_p_sq"]


# ---- the long partial lists of ba_hip_linearize ---------------------------------------------------------------
@pytest.mark.parametrize("n_landmarks", [sc.L1_THRESHOLD, sc.L1_THRESHOLD + 1], ids=["8192_partials", "8193_partials"])
def test_error_sum_on_both_sides_of_the_partial_threshold(n_landmarks):
    """proj_error of ba_hip_linearize against the long-double sum of the `r` tap (sqrt(w) r: test_step_path.py shows
    on the CPU that BuildProblem's sum is sum w |r|^2).  One partial per landmark; 8193 take k_sum_partials_l1.
    c: the kernel's term (r0^2 + r1^2) w has 4 roundings, the tap's (sqrt(w) r0)^2 + (sqrt(w) r1)^2 differs from it by
    4 more, the wavefront tree has 6 levels, then sum_partials (step_cases.chain without the block tree)."""
    c = sc.long_sums(n_landmarks)
    eng, _ = _engine(c)
    assert eng.structure_stats()["linearize_waves"] == n_landmarks
    got = eng.linearize().proj_error
    r = eng.get_proj_jacobians(c.O)[3]
    eng.end_solve()
    eng.close()
    want = (np.asarray(r, dtype=sc.LD) ** 2).sum()
    count = 4 + 4 + 6 + sc.chain(n_landmarks) - sc.TREE
    err = float(abs(sc.LD(got) - want) / (sc.EPS * want))
    print("STEP long_sums %d partials: proj_error %.17g against %.17g: %.3g eps of the sum (c = %d)"
          % (n_landmarks, got, float(want), err, count), flush=True)
    assert count < 64 and err <= count
