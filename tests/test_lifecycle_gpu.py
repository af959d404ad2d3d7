"""ba_hip_finalize drops what the engine held of the system before it (lifecycle.h, DESIGN.md "What the engine holds
and what drops it"): after solve_gn -> getters -> the same scene uploaded again -> finalize, every reader of the kept
factor refuses with the usual "needs the factor of the last ba_hip_solve_gn" message instead of reading the factor,
the selected inverse and its slot table of a system that is gone; after a new linearise and solve_gn the results are
those of the first round.  The second system has the size of the first on purpose: a stale read stays inside its
buffers, the test never needs an out-of-bounds access to fail.  Tolerance: max(1e-9, 4.5 eps cond(S)) of
leverage_cases.tolerance, covariances in correlation units (joint_state_cases.corr_err), hat blocks absolutely.

test_event_against_every_reader crosses every event of lifecycle_cases.EVENT_LIST with every reader of
lifecycle_cases.READERS on one engine per event.  What each cell must do is derived, not written down: the codes the
engine fires are replayed through ba_hostcheck_lifecycle and the reader's rule is applied to the bits
(lifecycle_cases.Tracker).  A refusal is matched with the wording of engine.hip; a reader served although nothing
rewrote the system returns the bits it returned before the event; a reader served after a new solve is compared with
a dense float64 reference built from the engine's own S, right-hand side and Jacobians of that solve.  Every engine
ends at state B (the same structure, every free pose moved): there each result must also lie more than 100 tolerances
from state A's, so that a stale read could not have passed.  Bounds: leverage_cases.tolerance for hat blocks and
solves, the same in correlation units for covariances, the eigenpair bound of test_weakest_modes_gpu, the two bounds
of pcg_panel_cases for the panel PCG (cond(S) rel_tolerance + 4.5 eps cond(S))."""
import numpy as np
import pytest

from ba_amd import hipapi, scene
from helpers import _add_pose_pose
from joint_state_cases import corr_err
import joint_state_cases as jc
import leverage_cases as lc
import lifecycle_cases as lcs
import pcg_panel_cases as ppc
import pplever_cases as pc

pytestmark = pytest.mark.gpu

P, L = 14, 60
REFUSED = "needs the factor of the last ba_hip_solve_gn \\(none yet, or the system was re-linearised since\\)"


def _scene():
    """LmSize 1, 14 poses of which the first two are fixed (72 pose rows: two tiles), 60 landmarks seen by 3 to 5
    poses each (the reference pose and 2 to 4 accepted residuals)"""
    sc = scene.make_scene(P, L, 4, lm_dim=1, seed=11, anchors=(0, 1))
    pa = np.ones(P, dtype=np.uint8)
    pa[:2] = 0
    k = np.arange(len(sc.obs_pose)) % 5          # 0: the reference observation (rejected), 1 .. 4 accepted
    keep = (k >= 1) & (k <= 2 + sc.obs_lm % 3)
    return sc, pa, (sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])


def _upload(eng, sc, pa, obs, pose_pose):
    """the whole problem into the engine, finalized (natural order)"""
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(*obs)
    if pose_pose:
        _add_pose_pose(eng, sc, P)
    eng.set_pose_ordering(hipapi.ORDER_NATURAL)
    eng.finalize()


def _solve(eng):
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(P, dtype=np.uint16))
    eng.linearize()
    assert eng.solve_gn() == 0


def _engine():
    eng = hipapi.Engine(1, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.keep_reduced_system = 1
    eng.set_options(o)
    return eng


def test_refinalize_drops_the_kept_factor():
    sc, pa, obs = _scene()
    nres = len(obs[1])
    assert set(np.bincount(obs[2], minlength=L)) == {2, 3, 4}
    lev_ids = [0, 7, nres // 2, nres - 1]
    getters = {
        "pose": lambda e: e.pose_marginals([2, 9]),
        "joint": lambda e: e.joint_marginals([3, 11]),
        "joint state": lambda e: e.joint_state_marginals([2, 9], [3, 40]),
        "leverages": lambda e: e.projection_leverages(lev_ids),
    }
    eng = _engine()
    _upload(eng, sc, pa, obs, False)
    _solve(eng)
    S = eng.get_S()
    assert S.shape == (72, 72)
    tol = lc.tolerance(S)
    first = {k: g(eng) for k, g in getters.items()}
    assert eng.marginal_stats()["store_tiles"] > 1   # (the slot table of the selected inverse is not trivial)
    eng.check_solve()

    _upload(eng, sc, pa, obs, False)   # the same system again: finalize re-allocates nothing
    for name, g in getters.items():
        with pytest.raises(hipapi.HipError, match=REFUSED):
            g(eng)
    with pytest.raises(hipapi.HipError, match="ba_hip_check_solve needs keep_reduced_system and a finished ba_hip_solve_gn"):
        eng.check_solve()
    # ba_hip_get_S takes its no-factor branch: it reads A (where the old factor still lies), not the kept copy of S
    assert not np.array_equal(eng.get_S(), S)

    _solve(eng)
    second = {k: g(eng) for k, g in getters.items()}
    errs = {
        "pose": max(corr_err(b, a) for a, b in zip(first["pose"], second["pose"])),
        "joint": corr_err(second["joint"], first["joint"]),
        "joint state": corr_err(second["joint state"], first["joint state"]),
        "leverages": float(np.abs(second["leverages"] - first["leverages"]).max()),
    }
    print("second round against the first: %s, tol %.3g, cond(S) %.3g" % (errs, tol, np.linalg.cond(S)))
    for name, err in errs.items():
        assert err <= tol, name
    assert np.abs(eng.get_S() - S).max() <= tol * np.abs(S).max()
    eng.close()


def test_refinalize_refuses_pose_pose_leverages():
    sc, pa, obs = _scene()
    eng = _engine()
    _upload(eng, sc, pa, obs, True)
    _solve(eng)
    cov, _, lev = eng.pose_pose_leverages(hipapi.RES_BINARY)
    assert np.all(np.isfinite(cov)) and lev[0] == 0 and np.all(lev[1:] > 0)   # (residual 0 joins the two fixed poses)
    _upload(eng, sc, pa, obs, True)
    for kind in (hipapi.RES_UNARY, hipapi.RES_BINARY):
        with pytest.raises(hipapi.HipError, match="ba_hip_get_pose_pose_leverages: " + REFUSED):
            eng.pose_pose_leverages(kind)
    _solve(eng)
    cov2, _, lev2 = eng.pose_pose_leverages(hipapi.RES_BINARY)
    assert np.abs(lev2 - lev).max() <= lc.tolerance(eng.get_S())
    eng.close()


# ---- every event against every reader (lifecycle_cases.py) -----------------------------------------------------
EPS = np.finfo(np.float64).eps
SEPARATION = 100.0


class _Setup:
    pass


def _upload_state(eng, ctx, poses, bad=False):
    """the whole problem with the poses of one state; bad: one residual names pose P, which the host rejects"""
    sc, z, pose, lm = ctx["sc"], *ctx["obs"]
    if bad:
        pose = pose.copy()
        pose[len(pose) // 2] = P
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(poses, is_active=ctx["pa"])
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(z, pose, lm)
    _add_pose_pose(eng, sc, P)
    eng.set_pose_ordering(hipapi.ORDER_NATURAL)


_pose_dz = {}


def _dz_at(ctx, poses):
    """the Jacobians of the pose-pose residuals from the oracle at the state `poses` (they depend on the poses alone)"""
    from test_pose_pose_leverages_gpu import _pose_jacobians
    key = poses.tobytes()
    if key not in _pose_dz:
        import copy
        sc = copy.copy(ctx["sc"])
        sc.poses = poses
        _pose_dz[key] = _pose_jacobians(sc, ctx["terms"], pa=ctx["pa"])[0]
        _pose_dz[key].setflags(write=False)
    return _pose_dz[key]


class _Refs:
    """the dense float64 references of one solve, from the engine's own S, right-hand side and Jacobians"""

    def __init__(self, eng, ctx):
        self.eng, self.ctx = eng, ctx
        self.S = eng.get_S()
        self.tol = lc.tolerance(self.S)
        self.cond = np.linalg.cond(self.S)
        self.Si = np.linalg.inv(self.S)
        self.d = np.sqrt(np.diag(self.Si))
        self.rhs = eng.get_rhs()[0]
        self.x = eng.get_delta_gn()[0]
        self.pcg_bound = self.cond * lcs.PCG_TOL + 4.5 * EPS * self.cond
        self.rows = lc.natural_rows(ctx["pa"])
        s = _Setup()
        s.eng, s.sc, s.pa, s.lm_dim, s.tvs, s.D, s.K = eng, ctx["sc"], ctx["pa"], 1, False, 6, 0
        s.la = np.ones(L, dtype=np.uint8)
        s.obs_pose, s.obs_lm = (np.asarray(a, dtype=np.int64) for a in ctx["obs"][1:])
        s.masks = np.zeros(P, dtype=np.uint16)
        self.s = s
        self._cache = {}

    def rows_of(self, ids):
        return np.array([self.rows[p] + x for p in ids for x in range(6)])

    def want(self, what):
        if what not in self._cache:
            self._cache[what] = getattr(self, "_" + what)()
        return self._cache[what]

    def _pose(self):
        return (np.stack([self.Si[np.ix_(self.rows_of([p]), self.rows_of([p]))] for p in lcs.POSE_IDS]),)

    def _pair(self):
        return (np.stack([self.Si[np.ix_(self.rows_of([a]), self.rows_of([b]))] for a, b in zip(lcs.PAIR_A, lcs.PAIR_B)]),)

    def _landmark(self):
        from test_marginals_gpu import _landmark_reference
        return (_landmark_reference(self.s, self.S, lcs.LM_IDS),)

    def _joint(self):
        r = self.rows_of(lcs.JOINT_IDS)
        return (self.Si[np.ix_(r, r)],)

    _pcg_joint = _joint

    def _jacobian(self):
        if "J" not in self._cache:
            self._cache["J"] = lc.engine_jacobian(self.s)[0]
        return self._cache["J"]

    def _joint_state(self):
        J, n = self._jacobian(), self.S.shape[0]
        cols = jc.request_columns(1, 6, 0, self.ctx["pa"], self.s.la, lcs.POSE_IDS, lcs.LM_IDS)
        npose = 6 * len(lcs.POSE_IDS)
        Hi = jc.full_inverse_block(J.T @ J, self.S, n, cols[npose:])
        sel = np.concatenate([cols[:npose], n + np.arange(len(lcs.LM_IDS))])
        return (Hi[np.ix_(sel, sel)],)

    def _lever(self):
        return (lc.hfull_form(self.s, self.S, self._jacobian(), self.ctx["lev_ids"]),)

    def pp(self):
        """(reference covariances of every pose-pose residual, Cholesky factors G of the test's Lambda, R)"""
        if "pp" not in self._cache:
            from test_pose_pose_leverages_gpu import _unary_scales
            t, pa = self.ctx["terms"], self.ctx["pa"]
            dz = _dz_at(self.ctx, np.ascontiguousarray(self.eng.get_poses(P)[0]))
            info, w = pc.informations(t, un_scale=_unary_scales(self.eng, t.counts[0]))
            lam = info * w[:, None, None]
            G = pc.whitened_rows(t, 6, dz, lam, pa, self.s.masks)[2]
            self._cache["pp"] = (pc.reference_cov(t, 6, dz, pa, self.s.masks, self.Si), G, pc.res_dim(t, 6), lam)
        return self._cache["pp"]

    def _solve(self):
        return (self.Si @ lcs.RHS,)

    _pcg_solve = _solve


def _corr(got, want, da, db):
    return float((np.abs(got - want) / np.outer(da, db)).max())


def _distance(what, got, want, refs):
    """the reader's error measure between two results of it, in units of the reader's tolerance at refs' solve"""
    tol = refs.tol
    if what == "pose":
        return max(_corr(g, w, refs.d[refs.rows_of([p])], refs.d[refs.rows_of([p])])
                   for g, w, p in zip(got[0], want[0], lcs.POSE_IDS)) / tol
    if what == "pair":
        return max(_corr(g, w, refs.d[refs.rows_of([a])], refs.d[refs.rows_of([b])])
                   for g, w, a, b in zip(got[0], want[0], lcs.PAIR_A, lcs.PAIR_B)) / tol
    if what == "landmark":
        d = np.sqrt(refs.want("landmark")[0].reshape(-1))
        return float((np.abs(got[0] - want[0]).reshape(-1) / d ** 2).max()) / tol
    if what == "joint":
        d = refs.d[refs.rows_of(lcs.JOINT_IDS)]
        return _corr(got[0], want[0], d, d) / tol
    if what == "joint_state":
        d = np.sqrt(np.diag(refs.want("joint_state")[0]))
        return _corr(got[0], want[0], d, d) / tol
    if what == "lever":
        return float(np.abs(got[0] - want[0]).max()) / tol
    if what in ("pp_unary", "pp_binary"):
        _, G, R, _ = refs.pp()
        sl = refs.ctx["terms"].kind_slice(0 if what == "pp_unary" else 1)
        return pc.block_err(pc.whiten(got[0], G[sl], R[sl]), pc.whiten(want[0], G[sl], R[sl])) / tol
    if what == "solve":
        return float((np.linalg.norm(got[0] - want[0], axis=0) / np.linalg.norm(want[0], axis=0)).max()) / tol
    if what == "modes":
        return float(np.max(np.abs(got[0] - want[0]) / np.abs(want[0]))) / tol
    if what == "check":
        return abs(got[0][1] - want[0][1]) / want[0][1] / tol
    if what in ("S", "marg"):
        return float(np.abs(got[0] - want[0]).max() / np.abs(want[0]).max()) / tol
    if what == "pcg_solve":
        return float((np.linalg.norm(got[0] - want[0], axis=0) / np.linalg.norm(want[0], axis=0)).max()) / refs.pcg_bound
    if what == "pcg_joint":
        return float(np.linalg.norm(got[0] - want[0], 2) / np.linalg.norm(want[0], 2)) / refs.pcg_bound
    raise KeyError(what)


def _verify(reader, got, refs, bits):
    """a served result of a new system against its dense reference: the error in units of the tolerance (<= 1 asserted)"""
    what = reader.what
    assert all(np.all(np.isfinite(g)) for g in got), reader.name
    if what in ("pp_unary", "pp_binary"):
        cov, G, R, lam = refs.pp()
        sl = refs.ctx["terms"].kind_slice(0 if what == "pp_unary" else 1)
        err = _distance(what, got, (cov[sl],), refs)
        white = pc.whiten(got[0], G[sl], R[sl])
        err = max(err, max(abs(l - np.trace(w)) / 6 for l, w in zip(got[2], white)) / refs.tol)
        assert max(np.abs(i - l).max() / np.abs(l).max() for i, l in zip(got[1], lam[sl])) <= 1e-12
    elif what == "modes":
        from test_weakest_modes_gpu import _check
        w = _check(refs.S, got[0], got[1], refs.eng.mode_stats(), refs.tol)
        err = _distance(what, got, (w[:lcs.MODES],), refs)
    elif what == "check":
        nr = np.linalg.norm(refs.rhs)
        assert abs(got[0][1] - nr) <= 1e-12 * nr
        err = got[0][0] / (refs.tol * nr)
    elif what == "S":
        if not ({"factored", "pcg_solved"} & bits):
            if "lin" in bits:   # linearised and not solved: A holds the new S
                assert np.array_equal(got[0], got[0].T)
            return 0.0          # (after a finalize alone A holds no system yet: served, nothing to compare)
        assert np.array_equal(got[0], refs.S)
        err = np.linalg.norm(got[0] @ refs.x - refs.rhs) / (refs.tol * np.linalg.norm(refs.rhs))
    elif what == "marg":
        H = got[0]
        assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() > -1e-9 * np.abs(H).max()
        return 0.0
    elif what == "pcg_stats":
        assert got[0][1] == 1 and got[0][2] <= lcs.PCG_TOL, got[0]
        return 0.0
    elif what == "pcg_solve":
        worst = ppc.assert_panel_bounds(refs.S, refs.cond, np.asarray(lcs.RHS), got[0], lcs.PCG_TOL, range(lcs.RHS.shape[1]))
        err = worst[1] / refs.pcg_bound
    else:
        if what in ("joint", "pcg_joint", "joint_state"):
            assert np.array_equal(got[0], got[0].T)
        err = _distance(what, got, refs.want(what), refs)
    assert err <= 1.0, (reader.name, err)
    return err


ANALOGUE = {"pcg_solve": "solve", "pcg_joint": "joint", "solve": "pcg_solve", "joint": "pcg_joint"}


def _state_a_result(reader, before):
    """the reading of state A to keep away from: the reader's own, or that of its twin on the other solver"""
    by_what = {lcs.READER[n].what: v for n, v in before.items() if not n.endswith("_cold")}
    if reader.name in before:
        return before[reader.name]
    return by_what.get(ANALOGUE.get(reader.what))


class _Tally:
    def __init__(self):
        self.n = {"served": 0, "refused": 0, "unchanged": 0}
        self.worst = 0.0
        self.least_separation = np.inf


def _read_all(eng, ctx, tracker, tally, phase, refs=None, before=None, keep=None, away_from=None):
    """every reader once, in table order.  phase "before": served results go to `keep`, refusals are matched;
    "unchanged": a served result must equal before[reader] bit for bit; "new": it is verified against refs, and with
    away_from also kept SEPARATION tolerances away from state A's reading."""
    for r in lcs.READERS:
        if r.before:
            r.before(eng)
        out, bits = tracker.expect(r)
        if out[0] == "refuse":
            with pytest.raises(hipapi.HipError, match=out[2]):
                r.call(eng, ctx)
            tally.n["refused"] += 1
            continue
        got = r.call(eng, ctx)
        if keep is not None:
            keep[r.name] = got
        if phase == "unchanged" and r.name in before:
            assert len(got) == len(before[r.name])
            for g, b in zip(got, before[r.name]):
                assert g.tobytes() == b.tobytes(), "%s changed although nothing rewrote the system" % r.name
            tally.n["unchanged"] += 1
            continue
        tally.n["served"] += 1
        if refs is None:
            continue
        tally.worst = max(tally.worst, _verify(r, got, refs, bits))
        old = _state_a_result(r, away_from) if away_from is not None else None
        if old is not None and r.what not in ("pcg_stats",):
            sep = _distance(r.what, got, old, refs)
            tally.least_separation = min(tally.least_separation, sep)
            assert sep > SEPARATION, "%s: %.3g tolerances from state A's result" % (r.name, sep)


def _solve_again(eng, tracker, full):
    if full:
        eng.begin_solve()
        eng.set_pose_masks(np.zeros(P, dtype=np.uint16))
        tracker.fire("solve_begins", "masks_changed")
    eng.linearize()
    tracker.fire(*lcs.LINEARIZE)
    assert eng.solve_gn() == 0


@pytest.fixture(scope="module")
def ctx():
    sc, pa, obs, poses_a, poses_b = lcs.scene_AB()
    nres = len(obs[1])
    lms = set(int(l) for p, l in zip(obs[1], obs[2]) if int(p) == lcs.MARG_POSE)
    lms |= set(int(l) for l in range(L) if int(sc.lm_ref_pose[l]) == lcs.MARG_POSE)
    return {"sc": sc, "pa": pa, "obs": obs, "poses_a": poses_a, "poses_b": poses_b, "upload": None,
            "lev_ids": [0, 7, nres // 2, nres - 1], "marg_lms": sorted(lms), "cam_params": sc.cam_params,
            "terms": pc.helper_terms(sc, P)}


@pytest.mark.parametrize("name", [ev.name for ev in lcs.EVENT_LIST])
def test_event_against_every_reader(ctx, name):
    ev = lcs.EVENT[name]
    ctx = dict(ctx, upload=lambda e, poses, bad: _upload_state(e, ctx, poses, bad))
    eng = _engine()
    tally = _Tally()
    tracker = lcs.Tracker()
    # the first round at state A, and the readings before the event
    _upload_state(eng, ctx, ctx["poses_a"])
    eng.finalize()
    if ev.setup == "pcg":
        eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=lcs.PCG_TOL)
    _solve(eng)
    if ev.setup == "direct":
        eng.compute_marginals()
    tracker.fire(*lcs.SETUPS[ev.setup])
    before = {}
    refs_a = _Refs(eng, ctx) if name.endswith("first_solve") else None
    _read_all(eng, ctx, tracker, _Tally() if refs_a is None else tally, "new", refs=refs_a, keep=before)
    # the event, and every reader after it
    ev.run(eng, ctx)
    tracker.fire(*ev.codes)
    rewritten = any(c in lcs.REWRITES for c in ev.codes)
    solved = {"factored", "pcg_solved"} & tracker.bits()
    _read_all(eng, ctx, tracker, tally, "new" if rewritten else "unchanged",
              refs=_Refs(eng, ctx) if rewritten and solved else None, before=before)
    # a fresh linearise and solve_gn serves again (no finalize in between unless the event was one)
    if ev.restore:
        ev.restore(eng, ctx)
        tracker.fire(*[c for c in ev.codes if c in ("masks_changed", "pose_cam_params_changed")])
    if "finalized" not in tracker.bits():
        _upload_state(eng, ctx, ctx["poses_a"])
        eng.finalize()
        tracker.fire(*lcs.UPLOAD, *lcs.FINALIZE)
    moved = "step_applied_to_1" in ev.codes and "rolled_back" not in ev.codes
    _solve_again(eng, tracker, full="finalize_begins" in tracker.codes[len(lcs.SETUPS[ev.setup]):])
    pcg_now = ev.setup == "pcg"   # (the events that switch the solver themselves put the direct one back)
    tracker.fire(*(lcs.PCG if pcg_now else lcs.DIRECT))
    _read_all(eng, ctx, tracker, tally, "new", refs=_Refs(eng, ctx), away_from=before if moved else None)
    # state B: the same structure, every free pose moved; first the direct solver, then PCG
    eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
    _upload_state(eng, ctx, ctx["poses_b"])
    eng.finalize()
    tracker.fire(*lcs.UPLOAD, *lcs.FINALIZE)
    _solve_again(eng, tracker, full=True)
    tracker.fire(*lcs.DIRECT)
    refs_b = _Refs(eng, ctx)
    assert np.array_equal(eng.get_poses(P)[0], ctx["poses_b"])
    _read_all(eng, ctx, tracker, tally, "new", refs=refs_b, away_from=before)
    eng.set_reduced_solver(hipapi.SOLVER_PCG, rel_tolerance=lcs.PCG_TOL)
    _solve_again(eng, tracker, full=False)
    tracker.fire(*lcs.PCG)
    _read_all(eng, ctx, tracker, tally, "new", refs=_Refs(eng, ctx), away_from=before)
    print("LIFECYCLE %s: served %d, refused %d, unchanged %d, worst err / tol %.3g (least separation from state A %.3g tol)"
          % (name, tally.n["served"], tally.n["refused"], tally.n["unchanged"], tally.worst, tally.least_separation))
    eng.close()


def test_calibration_marginals_through_the_events():
    """ba_hip_get_calibration_marginals (kept_factor_ready with its shorter wording) on a calibration engine of its
    own: DoTvs on the 44-pose scene of test_marginals_gpu, pose-pose terms keeping S well conditioned.  The events that
    apply there, one after the other on one engine; what each must do is derived as above."""
    from test_marginals_gpu import _blk_err, _engine as _calibration_engine, _solve as _relinearize_and_solve
    sc = scene.make_scene(44, 300, 6, lm_dim=1, seed=12)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    s = _calibration_engine(sc, 1, pa, tvs=True, pose_pose=True)   # set_calibration, upload, finalize, begin_solve, masks
    eng, r = s.eng, lcs.CALIBRATION_READER
    _relinearize_and_solve(s)
    t = lcs.Tracker(("calibration_changed",) + lcs.SETUP[:-1])
    count = {"served": 0, "refused": 0, "unchanged": 0}
    worst = [0.0]

    def read(same_as=None):
        out, _ = t.expect(r)
        if out[0] == "refuse":
            with pytest.raises(hipapi.HipError, match=out[2]):
                r.call(eng, None)
            count["refused"] += 1
            return None
        got = r.call(eng, None)[0]
        if same_as is not None:
            assert got.tobytes() == same_as.tobytes()
            count["unchanged"] += 1
            return got
        S = eng.get_S()
        err = _blk_err(got, np.linalg.inv(S)[-6:, -6:]) / lc.tolerance(S)
        worst[0] = max(worst[0], err)
        assert got.shape == (6, 6) and err <= 1.0, err
        count["served"] += 1
        return got

    def solve_again():
        eng.linearize()
        assert eng.solve_gn() == 0
        t.fire(*lcs.LINEARIZE, *lcs.DIRECT)
        return read()

    first = read()
    assert first is not None
    zeros = np.zeros(sc.num_poses, dtype=np.uint16)
    masks = zeros.copy()
    masks[int(np.nonzero(pa)[0][3])] = 0x7
    A, b = lcs._system()
    unchanged = [
        ("apply_step", lambda: lcs._step(eng), ("step_applied_to_1",)),
        ("rollback", eng.rollback, ("rolled_back",)),
        ("set_pose_masks", lambda: eng.set_pose_masks(masks), ("masks_changed",)),
        ("begin_solve", eng.begin_solve, ("solve_begins",)),
        ("pcg_solve", lambda: eng.pcg_solve(np.tril(A), b, 6, 1e-10), ("pcg_run_begins", "pcg_run_finished_plain")),
    ]
    for name, run, codes in unchanged:
        run()
        t.fire(*codes)
        assert read(same_as=first) is not None, name
    eng.set_pose_masks(zeros)
    t.fire("masks_changed")
    refusing = [
        ("dense_solve", lambda: eng.dense_solve(np.tril(A), b), ("standalone_factorisation",), "foreign factor"),
        ("tile_solve", lambda: eng.tile_solve(np.tril(A), b), ("standalone_factorisation",), "foreign factor"),
        ("linearize", eng.linearize, lcs.LINEARIZE, "no factor"),
        ("solve_gn_pcg", lambda: lcs._solve_pcg(eng, None), lcs.LINEARIZE + lcs.PCG, "PCG left no factor"),
        ("set_calibration", lambda: eng.set_calibration(0, True), ("calibration_changed",), "not finalized"),
    ]
    for name, run, codes, kind in refusing:
        run()
        t.fire(*codes)
        assert lcs.CALIBRATION_READER.rule(t.bits())[1] == kind, name
        assert read() is None, name
        eng.set_reduced_solver(hipapi.SOLVER_DIRECT)
        if "finalized" not in t.bits():
            eng.finalize()
            eng.begin_solve()
            eng.set_pose_masks(zeros)
            t.fire(*lcs.FINALIZE, "solve_begins", "masks_changed")
        assert solve_again() is not None, name
    # the same problem finalized again: the shorter "needs the factor" wording
    eng.set_poses(sc.poses, is_active=pa)
    eng.finalize()
    t.fire("problem_changed", *lcs.FINALIZE)
    assert read() is None
    print("LIFECYCLE calibration_marginals: served %d, refused %d, unchanged %d, worst err / tol %.3g"
          % (count["served"], count["refused"], count["unchanged"], worst[0]))
    eng.close()
