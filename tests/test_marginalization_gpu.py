"""Sliding-window marginalisation (ba_hip_marginalize) and the dense pose prior residual (ba_hip_set_dense_priors)
on the MI355X, checked by the identity that makes the two halves exact: the system "everything not absorbed, plus
the prior", linearised at the same state, is the full system with M and L eliminated.  Engine F holds the full
problem; engine R the same state with the absorbed residuals removed, M and L inactive and the prior added.
Tolerance: max(1e-9, 4.5 eps cond(S)) relative."""
import numpy as np
import pytest

from ba_amd import hipapi, scene
from helpers import _p, dp, u32p, u8p

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


class Prob:
    """One problem: scene state, the residual lists, activity flags."""


def make_problem(LM, D, P=12, nlm=40, imu=False, pose_pose=False, seed=5, outlier_frac=0.02):
    rng = np.random.default_rng(seed)
    pr = Prob()
    pr.LM, pr.D, pr.P = LM, D, P
    sc = scene.make_scene(P, max(nlm, 1), 4, lm_dim=max(LM, 1), seed=seed, outlier_frac=outlier_frac)
    if imu:
        scene.add_inertial(sc, seed=seed)
    pr.sc = sc
    pr.pa = np.ones(P, dtype=np.uint8)
    pr.pa[sc.anchor_poses] = 0
    pr.vel = sc.init_vel if imu else np.zeros((P, 3))
    pr.bias = 0.01 * rng.normal(size=(P, 6)) if imu else np.zeros((P, 6))
    if LM:
        nsel = sc.obs_per_landmark + (1 if LM == 1 else 0)
        sel = np.ones(len(sc.obs_pose), dtype=bool)
        if LM == 1:
            sel[::nsel] = False
        pr.z, pr.opose, pr.olm = sc.obs_z[sel], sc.obs_pose[sel].astype(np.uint32), sc.obs_lm[sel].astype(np.uint32)
        pr.la = np.ones(sc.num_landmarks, dtype=np.uint8)
    else:
        pr.z, pr.opose, pr.olm = np.zeros((0, 2)), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        pr.la = np.zeros(0, dtype=np.uint8)
    # pose-pose residuals
    pr.un = np.zeros(0, np.uint32)
    pr.b1 = pr.b2 = np.zeros(0, np.uint32)
    pr.i1 = pr.i2 = np.zeros(0, np.uint32)
    if pose_pose:
        pr.un = np.arange(0, P, 4, dtype=np.uint32)
        pr.un_t = np.ascontiguousarray(sc.gt_poses[pr.un] + np.r_[0.01 * rng.normal(size=3), 0, 0, 0, 0])
        pr.un_t[:, 3:7] /= np.linalg.norm(pr.un_t[:, 3:7], axis=1, keepdims=True)
        pr.un_ci = np.ascontiguousarray(np.tile(np.diag([1e2] * 3 + [1e3] * 3).reshape(1, 36), (len(pr.un), 1)))
        pr.b1 = np.arange(0, P - 1, 2, dtype=np.uint32)
        pr.b2 = pr.b1 + 1
        nb = len(pr.b1)
        t12 = np.zeros((nb, 7))
        for k, (a, b) in enumerate(zip(pr.b1, pr.b2)):
            Ra = scene.quat_to_rot(sc.gt_poses[a, 3:7])
            t12[k, :3] = Ra.T @ (sc.gt_poses[b, :3] - sc.gt_poses[a, :3]) + 0.01 * rng.normal(size=3)
            t12[k, 3:7] = scene.quat_mul(sc.gt_poses[a, 3:7] * np.array([-1, -1, -1, 1]), sc.gt_poses[b, 3:7])
        pr.b_t = t12
        pr.b_ci = np.ascontiguousarray(np.tile(np.diag([50.0] * 6).reshape(1, 36), (nb, 1)))
        pr.b_cs = np.ascontiguousarray(np.tile(np.diag([np.sqrt(50.0)] * 6).reshape(1, 36), (nb, 1)))
    if imu:
        pr.i1 = np.arange(0, P - 1, dtype=np.uint32)
        pr.i2 = pr.i1 + 1
    return pr


def build(pr, obs=None, un=None, bn=None, im=None, pa=None, la=None, priors=(), mode=hipapi.ORDER_NATURAL,
          host_structure=False, state=None, masks=None):
    """An engine of `pr` restricted to the given residual index sets (None: all)."""
    sc, D = pr.sc, pr.D
    eng = hipapi.Engine(max(pr.LM, 0), D)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 0
    o.keep_reduced_system = 1
    o.gyro_sigma, o.accel_sigma = 5.3088444e-5, 0.001883649
    o.gyro_bias_sigma, o.accel_bias_sigma = 1.4125375e-4, 1.2589254e-2
    eng.set_options(o)
    sel = lambda s, n: np.arange(n) if s is None else np.asarray(s, dtype=np.int64)
    obs, un, bn, im = sel(obs, len(pr.opose)), sel(un, len(pr.un)), sel(bn, len(pr.b1)), sel(im, len(pr.i1))
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    poses, vel, bias, lms = (sc.poses, pr.vel, pr.bias, sc.landmarks) if state is None else state
    eng.set_poses(poses, v_w=vel, b=bias, is_active=pr.pa if pa is None else pa)
    if pr.LM:
        eng.set_landmarks(lms, sc.lm_ref_pose, is_active=pr.la if la is None else la)
        eng.set_projection_residuals(pr.z[obs], pr.opose[obs], pr.olm[obs])
    if len(un):
        ids = np.ascontiguousarray(pr.un[un])
        t, ci = np.ascontiguousarray(pr.un_t[un]), np.ascontiguousarray(pr.un_ci[un])
        rot = np.ones(len(un), np.uint8)
        eng._chk(eng.L.ba_hip_set_unary_residuals(eng.h, len(un), _p(ids, u32p), _p(t, dp), _p(ci, dp), _p(rot, u8p)))
    if len(bn):
        p1, p2 = np.ascontiguousarray(pr.b1[bn]), np.ascontiguousarray(pr.b2[bn])
        t, ci, cs = (np.ascontiguousarray(a[bn]) for a in (pr.b_t, pr.b_ci, pr.b_cs))
        w, rot = np.ones(len(bn)), np.ones(len(bn), np.uint8)
        eng._chk(eng.L.ba_hip_set_binary_residuals(eng.h, len(bn), _p(p1, u32p), _p(p2, u32p), _p(t, dp), _p(ci, dp),
                                                   _p(cs, dp), _p(w, dp), _p(rot, u8p)))
    if len(im):
        p1, p2 = np.ascontiguousarray(pr.i1[im]), np.ascontiguousarray(pr.i2[im])
        meas = [sc.imu_meas[i] for i in im]
        ptr = np.zeros(len(im) + 1, np.uint32)
        ptr[1:] = np.cumsum([len(m) for m in meas])
        m7 = np.ascontiguousarray(np.concatenate(meas))
        w = np.ones(len(im))
        eng._chk(eng.L.ba_hip_set_gravity(eng.h, _p(np.ascontiguousarray(sc.gravity, dtype=np.float64), dp)))
        eng._chk(eng.L.ba_hip_set_imu_residuals(eng.h, len(im), _p(p1, u32p), _p(p2, u32p), _p(ptr, u32p), _p(m7, dp),
                                                _p(w, dp)))
    if priors:
        eng.set_dense_priors(list(priors))
    if host_structure:
        eng.debug_set(5, 1)
    eng.set_pose_ordering(mode)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(pr.P, dtype=np.uint16) if masks is None else masks)
    return eng


def absorbed(pr, M, L):
    """index sets of the residuals that stay (not absorbed) and the dropped observations"""
    M, L = set(int(x) for x in M), set(int(x) for x in L)
    keep_obs = [a for a in range(len(pr.opose)) if int(pr.olm[a]) not in L and int(pr.opose[a]) not in M]
    dropped = [a for a in range(len(pr.opose)) if int(pr.olm[a]) not in L and int(pr.opose[a]) in M]
    keep_un = [i for i in range(len(pr.un)) if int(pr.un[i]) not in M]
    keep_bn = [i for i in range(len(pr.b1)) if int(pr.b1[i]) not in M and int(pr.b2[i]) not in M]
    keep_im = [i for i in range(len(pr.i1)) if int(pr.i1[i]) not in M and int(pr.i2[i]) not in M]
    return keep_obs, dropped, keep_un, keep_bn, keep_im


def landmarks_of(pr, M):
    """every active landmark observed by or anchored in M"""
    M = set(int(x) for x in M)
    L = set(int(l) for p, l in zip(pr.opose, pr.olm) if int(p) in M)
    if pr.LM == 1:
        L |= set(int(l) for l in range(len(pr.la)) if int(pr.sc.lm_ref_pose[l]) in M)
    return sorted(l for l in L if pr.la[l])


def rows_of(pa, ids, D):
    opt = np.cumsum(pa.astype(np.int64)) - 1
    return np.concatenate([np.arange(opt[p] * D, opt[p] * D + D) for p in ids]) if len(ids) else np.zeros(0, np.int64)


def schur(S, r, elim):
    keep = np.setdiff1d(np.arange(S.shape[0]), elim)
    Skk, Ske, See = S[np.ix_(keep, keep)], S[np.ix_(keep, elim)], S[np.ix_(elim, elim)]
    X = np.linalg.solve(See, Ske.T)
    return Skk - Ske @ X, r[keep] - X.T @ r[elim], keep


def tol_of(S):
    return max(1e-9, 4.5 * EPS * np.linalg.cond(S))


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def gn_min(eng, errs):
    dp_, dl = eng.get_delta_gn()
    _, rp, rl = eng.get_rhs()
    return errs.total() - rp @ dp_ - rl @ dl


CASES = {"lm1_d6": dict(LM=1, D=6), "lm3_d6": dict(LM=3, D=6),
         "lm1_d15_imu": dict(LM=1, D=15, imu=True),
         "lm0_d9_posegraph": dict(LM=0, D=9, imu=True, pose_pose=True),
         "lm0_d9_unary": dict(LM=0, D=9, imu=True, pose_pose=True, M=[4]),           # pose 4 carries a unary residual
         "lm1_d15_masked": dict(LM=1, D=15, imu=True, masks={5: 0x7e00, 4: 0x01c0})}  # biases of M, velocity of B


def _full(pr, M, L, **kw):
    F = build(pr, **kw)
    ef = F.linearize()
    mg = F.marginalize(M, L)
    SF = F.get_S()
    rF = F.get_rhs()[0]
    assert F.solve_gn() == 0
    return F, ef, mg, SF, rF


def _reduced(pr, M, L, mg, extra_drop=(), **kw):
    keep_obs, dropped, ku, kb, ki = absorbed(pr, M, L)
    pa = pr.pa.copy()
    pa[list(M)] = 0
    la = pr.la.copy()
    if len(L):
        la[list(L)] = 0
    prior = {k: mg[k] for k in ("pose_ids", "x0", "H", "b", "c")}
    R = build(pr, obs=keep_obs, un=ku, bn=kb, im=ki, pa=pa, la=la, priors=[prior], **kw)
    return R, pa, la


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("variant", ["natural", "auto", "host_structure"])
def test_schur_identity(case, variant):
    kw0 = dict(CASES[case])
    M = kw0.pop("M", [5])
    mk = kw0.pop("masks", {})
    pr = make_problem(**kw0)
    D = pr.D
    masks = np.zeros(pr.P, dtype=np.uint16)
    for p, m in mk.items():
        masks[p] = m
    L = landmarks_of(pr, M) if pr.LM else []
    F, ef, mg, SF, rF = _full(pr, M, L, masks=masks)
    assert mg["dropped_projection"] == 0
    assert mg["absorbed_unary"] == sum(int(p) in set(M) for p in pr.un)
    if mk:  # a masked parameter of the blanket has zero rows and columns in H
        for i, p in enumerate(mg["pose_ids"]):
            for bit in range(D):
                if masks[p] & (1 << bit):
                    assert not mg["H"][i * D + bit].any() and mg["b"][i * D + bit] == 0
    assert mg["absorbed_projection"] == sum(int(l) in set(L) for l in pr.olm)
    kw = {"mode": hipapi.ORDER_AUTO} if variant == "auto" else ({"host_structure": True} if variant == "host_structure" else {})
    kw["masks"] = masks
    R, pa, la = _reduced(pr, M, L, mg, **kw)
    er = R.linearize()
    SR = R.get_S()
    rR = R.get_rhs()[0]
    elim = rows_of(pr.pa, M, D)
    Ss, rs, keep = schur(SF, rF, elim)
    tol = tol_of(SF)
    assert rel(SR, Ss) <= tol, (rel(SR, Ss), tol)
    assert rel(rR, rs) <= tol, (rel(rR, rs), tol)
    assert R.solve_gn() == 0
    dF, dlF = F.get_delta_gn()
    dR, dlR = R.get_delta_gn()
    assert rel(dR, dF[keep]) <= tol
    if pr.LM:
        lopt = np.cumsum(pr.la.astype(np.int64)) - 1
        kept_l = [l for l in range(len(pr.la)) if pr.la[l] and la[l]]
        idx = np.concatenate([np.arange(lopt[l] * pr.LM, lopt[l] * pr.LM + pr.LM) for l in kept_l])
        assert rel(dlR, dlF[idx]) <= tol
    mF, mR = gn_min(F, ef), gn_min(R, er)
    assert abs(mF - mR) <= tol * max(abs(ef.total()), 1.0), (mF, mR)


def test_dropped_observations():
    # the binary residual (4, 5) determines pose 5 together with the two landmarks anchored in it
    pr = make_problem(1, 6, pose_pose=True)
    M = [5]
    L = [l for l in range(len(pr.la)) if int(pr.sc.lm_ref_pose[l]) == 5]
    keep_obs, dropped, _, _, _ = absorbed(pr, M, L)
    assert len(dropped) > 0
    F, ef, mg, _, _ = _full(pr, M, L)
    assert mg["dropped_projection"] == len(dropped)
    # the identity against F built without the dropped observations
    sel = [a for a in range(len(pr.opose)) if a not in set(dropped)]
    F2 = build(pr, obs=sel)
    F2.linearize()
    SF, rF = F2.get_S(), F2.get_rhs()[0]
    R, pa, la = _reduced(pr, M, L, mg)
    R.linearize()
    Ss, rs, _ = schur(SF, rF, rows_of(pr.pa, M, 6))
    tol = tol_of(SF)
    assert rel(R.get_S(), Ss) <= tol and rel(R.get_rhs()[0], rs) <= tol


def test_chaining_two_windows():
    pr = make_problem(1, 6, P=14)
    M1 = [4]
    L1 = landmarks_of(pr, M1)
    F, ef, mg1, SF, rF = _full(pr, M1, L1)
    R1, pa1, la1 = _reduced(pr, M1, L1, mg1)
    R1.linearize()
    M2 = [int(mg1["pose_ids"][0]) if int(mg1["pose_ids"][0]) != 0 else int(mg1["pose_ids"][1])]
    pr1 = pr
    L2 = [l for l in landmarks_of(pr, M2) if la1[l]]
    mg2 = R1.marginalize(M2, L2)
    assert mg2["absorbed_priors"] == 1
    # R2: everything touching M1 or M2 removed, the second prior only
    keep_obs, _, ku, kb, ki = absorbed(pr1, M1 + M2, sorted(set(L1) | set(L2)))
    pa = pr.pa.copy(); pa[M1 + M2] = 0
    la = pr.la.copy(); la[sorted(set(L1) | set(L2))] = 0
    prior = {k: mg2[k] for k in ("pose_ids", "x0", "H", "b", "c")}
    R2 = build(pr, obs=keep_obs, un=ku, bn=kb, im=ki, pa=pa, la=la, priors=[prior])
    R2.linearize()
    Ss, rs, _ = schur(SF, rF, rows_of(pr.pa, sorted(M1 + M2), 6))
    tol = tol_of(SF)
    assert rel(R2.get_S(), Ss) <= tol and rel(R2.get_rhs()[0], rs) <= tol


def test_pattern_and_marginals():
    pr = make_problem(1, 6)
    M = [5]
    L = landmarks_of(pr, M)
    F, ef, mg, SF, _ = _full(pr, M, L)
    R, pa, la = _reduced(pr, M, L, mg)
    R.linearize()
    assert R.solve_gn() == 0
    nz = R.factor_tile_pattern()
    opt = np.cumsum(pa.astype(np.int64)) - 1
    for p in mg["pose_ids"]:
        for p2 in mg["pose_ids"]:
            r0, c0 = opt[p] * 6, opt[p2] * 6
            for r in range(r0 // 64, (r0 + 5) // 64 + 1):
                for c in range(c0 // 64, (c0 + 5) // 64 + 1):
                    assert nz[max(r, c), min(r, c)]
    kept = [p for p in range(pr.P) if pa[p]]
    F.compute_marginals()
    R.compute_marginals()
    cF, cR = F.pose_marginals(kept), R.pose_marginals(kept)
    assert rel(cR, cF) <= max(1e-9, 4.5 * EPS * np.linalg.cond(SF))


def _gn(eng, iters):
    for _ in range(iters):
        eng.linearize()
        assert eng.solve_gn() == 0
        eng.compose_step(0.0, 1.0)
        eng.apply_step()


def _state(eng, pr):
    eng.end_solve()
    t, v, b = eng.get_poses(pr.P)
    return t, v, b, eng.get_landmarks(len(pr.la))


def test_sliding_window_prior_beats_dropping():
    """Slide once: Gauss-Newton steps on the whole window, then pose 1 and its landmarks leave.  Carried as a
    prior, the window stays at the batch solution of the whole trajectory; with them simply dropped it does not."""
    pr = make_problem(1, 6, P=14, nlm=150, seed=7, outlier_frac=0.0)
    batch = build(pr)
    _gn(batch, 12)
    xb = _state(batch, pr)[0]
    W = build(pr)
    _gn(W, 8)
    W.linearize()
    M = [1]
    L = landmarks_of(pr, M)
    mg = W.marginalize(M, L)
    st = _state(W, pr)
    keep_obs, _, ku, kb, ki = absorbed(pr, M, L)
    pa = pr.pa.copy(); pa[M] = 0
    la = pr.la.copy(); la[L] = 0
    prior = {k: mg[k] for k in ("pose_ids", "x0", "H", "b", "c")}
    out = {}
    for name, priors in (("prior", [prior]), ("dropped", [])):
        R = build(pr, obs=keep_obs, un=ku, bn=kb, im=ki, pa=pa, la=la, priors=priors, state=st)
        _gn(R, 12)
        x = _state(R, pr)[0]
        kept = np.flatnonzero(pa)
        out[name] = np.nan_to_num(np.sqrt(np.mean(np.sum((x[kept, :3] - xb[kept, :3]) ** 2, axis=1))), nan=np.inf)
    assert out["prior"] < 0.2 * out["dropped"], out
    assert out["prior"] < 1e-6, out


def _np_delta(x0, x, D):
    qc = x[3:7] * np.array([-1, -1, -1, 1])
    r = scene.quat_mul(qc, x0[3:7])
    r = r / np.linalg.norm(r)
    n = np.linalg.norm(r[:3])
    w = 2 * np.arctan2(n, r[3]) / n * r[:3] if n > 1e-12 else 2 * r[:3] / r[3]
    return np.concatenate([x0[:3] - x[:3], w, x0[7:7 + D - 6] - x[7:7 + D - 6]])


def _np_apply(x, delta, D):
    y = x.copy()
    y[:3] -= delta[:3]
    q = scene.quat_mul(x[3:7], scene.quat_exp(-delta[3:6]))
    y[3:7] = q / np.linalg.norm(q)
    y[7:7 + D - 6] -= delta[6:D]
    return y


@pytest.mark.parametrize("D", [6, 15])
def test_prior_away_from_x0(D):
    """A prior alone on three poses, state away from x0: S, rhs, E_p and the dogleg term against numpy and
    central differences of E_p."""
    rng = np.random.default_rng(D)
    P, k = 3, 3
    x = np.zeros((P, 16))
    x[:, :3] = rng.normal(size=(P, 3))
    q = rng.normal(size=(P, 4))
    x[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x[:, 7:] = 0.1 * rng.normal(size=(P, 9))
    x0 = np.array([_np_apply(x[i], 0.05 * rng.normal(size=D), D) for i in range(P)])
    A = rng.normal(size=(k * D, k * D))
    H = A @ A.T + k * D * np.eye(k * D)
    b = rng.normal(size=k * D)
    c = 3.0
    eng = hipapi.Engine(0, D)
    o = hipapi.Options()
    o.keep_reduced_system = 1
    eng.set_options(o)
    eng.set_cameras(np.array([[500.0, 500.0, 320.0, 240.0]]), [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(x[:, :7], v_w=x[:, 7:10], b=x[:, 10:16], is_active=np.ones(P, np.uint8))
    eng.set_dense_priors([{"pose_ids": np.arange(P), "x0": x0, "H": H, "b": b, "c": c}])
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(P, dtype=np.uint16))
    errs = eng.linearize()
    S = eng.get_S()
    _, rhs, _ = eng.get_rhs()

    def energy(xs):
        d = np.concatenate([_np_delta(x0[i], xs[i], D) for i in range(P)])
        return c - 2 * b @ d + d @ H @ d

    E = energy(x)
    assert abs(errs.unary_error - E) <= 1e-9 * abs(E)
    assert abs(eng.eval_residuals().unary_error - E) <= 1e-9 * abs(E)
    assert abs(eng.prior_errors(1)[0] - E) <= 1e-9 * abs(E)
    h = 1e-6
    n = P * D
    g = np.zeros(n)
    Jfd = np.zeros((n, n))
    for kk in range(n):
        e = np.zeros(n)
        e[kk] = h
        xp = np.array([_np_apply(x[i], e[i * D:(i + 1) * D], D) for i in range(P)])
        xm = np.array([_np_apply(x[i], -e[i * D:(i + 1) * D], D) for i in range(P)])
        g[kk] = -(energy(xp) - energy(xm)) / (2 * h) / 2
        dpl = np.concatenate([_np_delta(x0[i], xp[i], D) for i in range(P)])
        dmi = np.concatenate([_np_delta(x0[i], xm[i], D) for i in range(P)])
        Jfd[:, kk] = (dpl - dmi) / (2 * h)
    assert rel(rhs, g) <= 1e-6, rel(rhs, g)
    Sfd = Jfd.T @ H @ Jfd
    assert rel(S, Sfd) <= 1e-6, rel(S, Sfd)
    # the dogleg denominator: |J rhs|^2 = rhs^T S rhs for a prior alone
    dl = eng.dogleg_terms(0)
    assert abs(dl.j_rhs_sq - rhs @ S @ rhs) <= 1e-9 * abs(rhs @ S @ rhs)


def test_determinism_symmetry_and_refusals():
    pr = make_problem(1, 6)
    M = [5]
    L = landmarks_of(pr, M)
    F = build(pr)
    F.linearize()
    a = F.marginalize(M, L)
    b = F.marginalize(M, L)
    for key in ("H", "b", "x0"):
        assert np.array_equal(a[key], b[key])
    assert a["c"] == b["c"]
    assert np.array_equal(a["H"], a["H"].T)
    assert np.all(np.linalg.eigvalsh(a["H"]) > -1e-9 * np.abs(a["H"]).max())
    bad = [([], L), ([5, 5], L), ([99], L), ([0], []),          # empty, twice, unknown, inactive (anchor)
           ([5], L + [999]), ([5], L + [L[0]]),                 # unknown landmark, landmark twice
           ([5], [l for l in L if int(pr.sc.lm_ref_pose[l]) != 5])]  # a landmark anchored in M missing
    for m, l in bad:
        with pytest.raises(hipapi.HipError):
            F.marginalize(m, l)
        # the engine stays usable
        c = F.marginalize(M, L)
        assert np.array_equal(c["H"], a["H"])
    # new masks, a rollback and a step all invalidate the linearisation
    F.set_pose_masks(np.zeros(pr.P, dtype=np.uint16))
    with pytest.raises(hipapi.HipError):
        F.marginalize(M, L)
    F.linearize()
    assert F.solve_gn() == 0
    F.compose_step(0.0, 1.0)
    F.apply_step()
    F.rollback()
    with pytest.raises(hipapi.HipError):
        F.marginalize(M, L)
    F.linearize()
    # S^a_MM not positive definite: pose 5 keeps only the landmarks anchored in it (the rest is dropped)
    with pytest.raises(hipapi.HipError, match="positive definite"):
        F.marginalize(M, [l for l in L if int(pr.sc.lm_ref_pose[l]) == 5])
    F.marginalize(M, L)
    # no linearisation of the current state after a step
    assert F.solve_gn() == 0
    F.compose_step(0.0, 1.0)
    F.apply_step()
    with pytest.raises(hipapi.HipError):
        F.marginalize(M, L)
    F.linearize()
    F.marginalize(M, L)
    F.release_marginalization()


def test_dense_priors_refused_with_calibration_unknowns():
    pr = make_problem(1, 6)
    eng = hipapi.Engine(1, 6)
    eng.set_calibration(0, True)
    eng.set_cameras(pr.sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(pr.sc.poses, is_active=pr.pa)
    eng.set_landmarks(pr.sc.landmarks, pr.sc.lm_ref_pose)
    eng.set_projection_residuals(pr.z, pr.opose, pr.olm)
    eng.set_dense_priors([{"pose_ids": [2], "x0": np.zeros((1, 16)) + np.r_[0, 0, 0, 0, 0, 0, 1, np.zeros(9)],
                           "H": np.eye(6), "b": np.zeros(6), "c": 0.0}])
    with pytest.raises(hipapi.HipError, match="calibration"):
        eng.finalize()
